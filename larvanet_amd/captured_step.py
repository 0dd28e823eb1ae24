"""The training step as hipGraphs.  One step issues ~330 short kernels; launched one by one from Python the GPU idles
between them, so forward + backward are captured once per (batch shape, early-loss mode) and replayed.  The plugin
(models/LarvaNet.py) holds at most one CapturedStep and replaces it only by another that was captured whole."""
import contextlib
import gc

import torch

from .autograd import DeferredWgrad, DualChain


class LossCopy:
    """How the "split" capture hands the loss to the host early: a pinned float, the side stream that copies the loss
    into it beside the backward graph, and the two events around that copy.  One per plugin."""

    def __init__(self):
        self.host = torch.empty((), dtype=torch.float32).pin_memory()
        self.stream = torch.cuda.Stream()
        self.done, self.fwd_done = torch.cuda.Event(), torch.cuda.Event()

    def start(self, loss):
        self.fwd_done.record()
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(self.fwd_done)
            self.host.copy_(loss, non_blocking=True)
            self.done.record()

    def result(self):
        self.done.synchronize()
        return self.host.item()


class CapturedStep:
    """What one capture produced.  mode False: one graph.  "poll": one graph whose loss-finishing launch also stores the
    loss into `handoff`, a kernels.HostCell, which the host polls.  "split": forward | backward as two graphs over one
    memory pool; the loss is complete when the first ends and `handoff`, a LossCopy, takes it out between them.  late:
    the graph of the second half of a split weight-gradient flush, or None."""

    def __init__(self, plugin, key, mode, handoff, input_tensor, truth_tensor):
        # built in locals and assigned at the end: a capture that raises leaves no half-made step behind
        x, truth = input_tensor.clone(), truth_tensor.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):  # warm-up outside capture (lazy kernel attributes, allocator pools)
                plugin._zero_grad()
                plugin._step_body(x, truth)
                DeferredWgrad.flush_late()
        torch.cuda.current_stream().wait_stream(side)
        plugin._zero_grad()
        gc.collect()   # (a dropped plugin's graphs must not be freed while a capture is open: inference._capture_infer)
        graph = torch.cuda.CUDAGraph()
        back = torch.cuda.CUDAGraph() if mode == "split" else None
        # thread_local: a process-group watchdog thread must not abort the capture
        with contextlib.ExitStack() as capturing:
            capturing.enter_context(torch.cuda.graph(graph, capture_error_mode="thread_local"))

            def cut():   # between forward and backward of the split mode: the first graph ends, the second begins
                DualChain.join()
                capturing.close()
                capturing.enter_context(torch.cuda.graph(back, pool=graph.pool(), capture_error_mode="thread_local"))
            # (the StepScope is left inside the last graph: that joins the chains and issues the queued weight gradients)
            loss, out, early_lo = plugin._step_body(x, truth, early_loss=handoff if mode == "poll" else bool(mode),
                                                    cut=cut if back is not None else None)
        late = None
        if DeferredWgrad.has_late():  # second half of a split backward: its own graph, same memory pool
            late = torch.cuda.CUDAGraph()
            with torch.cuda.graph(late, pool=graph.pool(), capture_error_mode="thread_local"):
                DeferredWgrad.flush_late()
        self.key, self.mode, self.handoff = key, mode, handoff
        self.static_in, self.static_truth = x, truth
        self.graph, self.back, self.late = graph, back, late
        self.loss, self.out, self.early_lo = loss, out, early_lo

    def stage(self, input_tensor, truth_tensor):
        """The batch into the step's input buffers (train_larva.py:123-128 hands over fresh device tensors every step), on
        the current stream, i.e. ordered behind whatever produced them (on a stream of their own the two cross-stream
        waits cost more than the two 5 us copies they hide).  A producer that filled buffers() in place hands the very
        same storage back: nothing to copy."""
        for dst, src in ((self.static_in, input_tensor), (self.static_truth, truth_tensor)):
            if src.data_ptr() != dst.data_ptr():
                dst.copy_(src)

    def replay(self):
        """-> (loss, last output, the late graph's replay or None).  The two tensors are the graphs' own buffers; the
        gradients are overwritten in place: no zero_grad needed."""
        if self.mode == "poll":
            self.handoff.expect()   # this replay's store carries the next sequence number
        self.graph.replay()
        if self.back is not None:
            self.handoff.start(self.loss)   # the loss goes to pinned host memory on a stream of its own while backward runs
            self.back.replay()
        return self.loss, self.out, self.late.replay if self.late is not None else None

    def buffers(self, input_shape, truth_shape):
        """(static input, static truth) if they have these shapes, else None."""
        fits = tuple(self.static_in.shape) == tuple(input_shape) and tuple(self.static_truth.shape) == tuple(truth_shape)
        return (self.static_in, self.static_truth) if fits else None
