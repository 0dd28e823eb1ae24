"""The order in which launches on different streams touch the same memory (tests/stream_order.py holds the checker and
the recorder; its docstring states the model).

CPU: the checker on hand-written logs, and the footprint table against include/larva_hip.h.
GPU: each scenario runs ONCE under the recorder, at the 5 x 3 x 16 x 20 batch at which the two half-batch chains really
fork, and its log is checked on the host; the audit is then shown to bite by taking ordering records out of those logs
(never out of the program).  Every scenario asserts that it launched on at least two streams and captured / replayed what
it was meant to: one that silently ran single-stream fails.
"""
import gc
import importlib
import types

import numpy as np
import pytest
import torch

import stream_order as SO
from stream_order import access, capture_begin, capture_end, check, host_access, host_sync, record, replay, wait, wait_stream

A, B, C = 0x1000, 0x2000, 0x3000     # three buffers of 0x100 bytes
MAIN, SIDE, COPY = 0, 7, 9


def buf(base, label, lo=0, hi=0x100):
    return [(base + lo, base + hi, label)]


# ------------------------------------------------------------------------------------------------ the checker (CPU)
def _ordered_by_event():
    return [access(SIDE, "produce", writes=buf(A, "out")), record("e", SIDE), wait(MAIN, "e"), access(MAIN, "consume", reads=buf(A, "x"))]


def test_two_streams_ordered_by_an_event_pass():
    assert check(_ordered_by_event()) == []


def test_the_same_log_without_the_wait_is_reported():
    log = _ordered_by_event()
    (c,) = check(SO.drop_record(log, 2))
    assert c.names() == {"produce", "consume"} and c.streams() == {MAIN, SIDE} and c.labels() == {"out", "x"}
    assert (c.lo, c.hi) == (A, A + 0x100) and (c.first["index"], c.second["index"]) == (0, 2) and c.kind() == "RaW"
    assert "produce.out" in repr(c) and "consume.x" in repr(c)


def test_a_wait_on_an_event_recorded_before_the_conflicting_launch_is_reported():
    log = [record("e", SIDE), access(SIDE, "produce", writes=buf(A, "out")), wait(MAIN, "e"), access(MAIN, "consume", reads=buf(A, "x"))]
    (c,) = check(log)
    assert c.names() == {"produce", "consume"}


def _two_halves(join_first):
    fork = wait_stream(SIDE, MAIN, "fork")
    halves = [access(MAIN, "conv", writes=buf(A, "out", 0, 0x80)), access(SIDE, "conv", writes=buf(A, "out", 0x80, 0x100))]
    join, reader = wait_stream(MAIN, SIDE, "join"), [access(MAIN, "exits", reads=buf(A, "fea"))]
    return fork + halves + (join + reader if join_first else reader + join)


def test_half_tensor_writers_and_a_whole_tensor_reader_behind_the_join_pass():
    assert check(_two_halves(True)) == []


def test_a_join_below_the_whole_tensor_reader_is_reported_for_the_second_half_only():
    (c,) = check(_two_halves(False))
    assert (c.lo, c.hi) == (A + 0x80, A + 0x100) and c.first["stream"] == SIDE and c.second["name"] == "exits"


@pytest.mark.parametrize("first,second,kind", [("writes", "reads", "RaW"), ("reads", "writes", "WaR"), ("writes", "writes", "WaW")])
def test_each_kind_of_hazard_is_reported(first, second, kind):
    log = [access(MAIN, "one", **{first: buf(A, "p")}), access(SIDE, "two", **{second: buf(A, "q", 0x40, 0x140)})]
    (c,) = check(log)
    assert c.kind() == kind and (c.lo, c.hi) == (A + 0x40, A + 0x100)
    assert check([access(MAIN, "one", reads=buf(A, "p")), access(SIDE, "two", reads=buf(A, "q"))]) == []   # two readers


def test_a_write_is_checked_against_the_readers_of_every_stream_since_the_last_write():
    log = [access(MAIN, "w", writes=buf(A, "p")), host_sync(), access(MAIN, "r0", reads=buf(A, "p")), access(SIDE, "r1", reads=buf(A, "p")),
           access(COPY, "w2", writes=buf(A, "p"))]
    assert sorted(c.first["name"] for c in check(log)) == ["r0", "r1"]


def test_a_conflict_hidden_by_a_host_sync_passes():
    for sync in (host_sync(stream=SIDE), host_sync(), None):
        log = [access(SIDE, "produce", writes=buf(A, "out")), sync, access(MAIN, "consume", reads=buf(A, "x"))]
        assert len(check([r for r in log if r])) == (0 if sync else 1)
    log = [access(SIDE, "produce", writes=buf(A, "out")), record("e", SIDE), host_sync(event="e"), access(COPY, "consume", reads=buf(A, "x"))]
    assert check(log) == []
    assert len(check(log[:1] + [host_sync(stream=MAIN)] + log[3:])) == 1      # the host waited for the wrong stream


def test_a_fork_inside_a_capture_that_does_not_rejoin_before_the_last_reader_is_reported():
    def body(joined):
        return ([capture_begin("g", MAIN)] + wait_stream(SIDE, MAIN, "f") + [access(SIDE, "conv", writes=buf(A, "out"))]
                + (wait_stream(MAIN, SIDE, "j") if joined else []) + [access(MAIN, "exits", reads=buf(A, "fea")), capture_end("g")])
    assert check(body(True)) == []
    (c,) = check(body(False))
    assert c.scope == "g" and c.names() == {"conv", "exits"}
    # the body does not run: nothing outside conflicts with it
    assert check([access(COPY, "other", writes=buf(A, "x"))] + body(True)) == []


def test_a_replay_and_a_reader_of_its_static_output_on_another_stream_need_an_edge():
    body = [capture_begin("g", SIDE), access(SIDE, "net", reads=buf(A, "static_in"), writes=buf(B, "static_out")), capture_end("g")]
    use = [access(MAIN, "stage", writes=buf(A, "dst")), replay("g", MAIN)]
    reader = [access(COPY, "d2h", reads=buf(B, "src"), writes=buf(C, "pinned"))]
    (c,) = check(body + use + reader)
    assert c.names() == {"replay(g)", "d2h"} and c.labels() == {"net.static_out", "src"}
    assert check(body + use + wait_stream(COPY, MAIN, "fwd") + reader) == []
    with pytest.raises(ValueError, match="never captured"):
        check(use)


def test_a_host_access_before_the_copy_that_fills_the_range_was_waited_for_is_reported():
    d2h = [access(COPY, "d2h", reads=buf(B, "dev"), writes=buf(C, "pinned")), record("done", COPY)]
    (c,) = check(d2h + [host_access(reads=buf(C, "pin.out"))])
    assert c.names() == {"d2h", "host"} and c.labels() == {"pinned", "pin.out"}
    assert check(d2h + [host_sync(event="done"), host_access(reads=buf(C, "pin.out"))]) == []
    # the host writing a pinned buffer a copy still reads; work issued after a host access is behind it
    h2d = [access(COPY, "h2d", reads=buf(C, "pinned"), writes=buf(B, "dev"))]
    assert len(check(h2d + [host_access(writes=buf(C, "pin.in"))])) == 1
    assert check([host_access(writes=buf(C, "pin.in"))] + h2d) == []


def test_the_allocators_record_stream_rule():
    """A block that was record_stream'ed is reused only behind the recorded stream's work up to its release."""
    log = [access(MAIN, "fill", writes=buf(A, "dev")), SO.record_stream(A, A + 0x100, COPY)] + wait_stream(COPY, MAIN, "h") + \
          [access(COPY, "d2h", reads=buf(A, "dev")), SO.free(A, A + 0x100), access(MAIN, "next owner", writes=buf(A, "new"))]
    assert check(log) == []
    assert len(check([r for r in log if r["kind"] != "free"])) == 1           # still alive: nothing guards the overwrite
    assert len(check(log + [access(COPY, "late", reads=buf(A, "dev"))])) == 1   # and the guard covers one reuse, not later work


def test_a_launch_of_an_entry_point_without_a_footprint_raises_by_name():
    from larvanet_amd import hip_lib
    params = SO.parse_params(hip_lib.HEADER_PATH)
    name = "larva_sum_scalars"
    assert name not in SO.FOOTPRINTS and SO.is_launch(params[name])
    with pytest.raises(SO.MissingFootprint, match=name):
        SO.launch_record(name, params[name], (hip_lib.ptr_array([A]), 1, 1.0, B, None))
    # and a declared one gives the operands their const-ness and extents
    r = SO.launch_record("larva_upsample4_fwd", params["larva_upsample4_fwd"], (A, B, 2, 3, 4, 5, 0, SIDE))
    assert r["stream"] == SIDE and r["reads"] == [[A, A + 4 * 2 * 3 * 4 * 5, "in"]] and r["writes"] == [[B, B + 64 * 2 * 3 * 4 * 5, "out"]]
    with pytest.raises(SO.MissingFootprint, match="larva_upsample4_fwd.*`out`"):
        SO.launch_record("larva_upsample4_fwd", params["larva_upsample4_fwd"], (A, B, 2, 3, 4, 5, 0, None),
                         footprints={"larva_upsample4_fwd": {"dev": {"in": lambda a: 4}, "host": ()}})


def test_the_footprint_table_agrees_with_the_header():
    from larvanet_amd import hip_lib
    params = SO.parse_params(hip_lib.HEADER_PATH)
    assert set(params) == set(hip_lib.SIGNATURES)
    for name, ps in params.items():
        assert len(ps) == len(hip_lib.SIGNATURES[name][1]), name
    for name, fp in SO.FOOTPRINTS.items():
        assert name in hip_lib.SIGNATURES, "%s is not an entry point of the header" % name
        assert SO.is_launch(params[name]), "%s takes no stream" % name
        pointers = {p.name for p in params[name] if p.pointer and not p.stream}
        declared = set(fp["dev"]) | set(fp["host"])
        assert not (set(fp["dev"]) & set(fp["host"])), name
        assert pointers - declared == set(), "%s: no extent for %s" % (name, sorted(pointers - declared))
        assert declared - pointers == set(), "%s: the header has no pointer parameter %s" % (name, sorted(declared - pointers))
    src = {p.name: p.const for p in params["larva_conv3x3_fwd_strips"]}
    assert src["src"] and src["wpk"] and not src["out"]
    pk = {p.name: p.const for p in params["larva_pack_weights_batch"]}
    assert pk["w"] and not pk["wpk_fwd"] and not pk["wpk_bwd"]


# ------------------------------------------------------------------------------------------------ the scenarios (GPU)
ARGS = types.SimpleNamespace(train_path="/tmp")
V1 = ("LarvaNet", ["--num_modules=3", "--num_blocks=2,1,2"])
V2 = ("LarvaNetV2", ["--num_modules=2", "--num_blocks=1,2"])


class NoValidation:
    """train_step_larva validates after its first step: over no images here."""

    def get_num_images(self):
        return 0


def _plugin(name, flags, training, extra=(), **attrs):
    m = importlib.import_module("larvanet_amd.models." + name).create_model()
    m.parse_args(list(flags) + list(extra))
    m.strict_graph = True
    torch.manual_seed(5)
    m.prepare(is_training=training, scales=[4])
    for k, v in attrs.items():
        assert hasattr(m, k), k
        setattr(m, k, v)
    return m


def _batches(device, n):
    g = torch.Generator().manual_seed(23)
    return [((torch.rand(5, 3, 16, 20, generator=g) * 255).to(device), (torch.rand(5, 3, 64, 80, generator=g) * 255).to(device))
            for _ in range(n)]


def _train(network, **attrs):
    def run(rec, device):
        m = _plugin(*network, True, **attrs)
        for x, t in _batches(device, 3):
            loss = m.train_step_larva(ARGS, NoValidation(), x, t)
            assert isinstance(loss, float) and np.isfinite(loss)
        assert m.use_hip_graph == attrs["use_hip_graph"] and m.hip_graph_fell_back is None
    return run


def _loader_into_step(rec, device):
    from larvanet_amd.dataloaders import device_patch_loader as D
    ld = D.create_loader()
    ld.parse_args(["--device_source=synthetic_loader", "--synthetic_images=3", "--synthetic_lr_size=40", "--data_seed=3"])
    ld.prepare([4])
    m = _plugin(*V1, True, use_hip_graph=True)
    shapes = ((5, 3, 16, 16), (5, 3, 64, 64))
    in_place = 0
    for _ in range(3):
        bufs = m.input_buffers(*shapes)
        x, t = ld.get_device_batch(5, 4, 16, out=bufs)
        in_place += bufs is not None and x.data_ptr() == bufs[0].data_ptr()
        m.train_step_larva(ARGS, NoValidation(), x, t)
    assert in_place == 2, "the loader never wrote into the captured step's buffers"


def _images(n, channels=3, h=16, w=20):
    rng = np.random.RandomState(11)
    out = [rng.randint(0, 256, size=(h, w, channels)).astype(np.uint8) for _ in range(n)]
    if channels == 4:
        out[1][..., 3] = 255     # one opaque image among the transparent ones
    return out


def _upscale(precision, n=5, **kw):
    def run(rec, device):
        from larvanet_amd import pipeline
        m = _plugin(*V1, False, extra=["--precision=" + precision])
        images = _images(n, 4 if kw.get("keep_alpha") else 3)
        got = list(pipeline.upscale_stream(m, images, 4, depth=2, **kw))
        assert len(got) == n and all(g.dtype == np.uint8 for g in got)
    return run


def _video(rec, device):
    from larvanet_amd import pipeline
    from larvanet_amd.image_utils import i420_frame_bytes
    m = _plugin(*V1, False)
    rng = np.random.RandomState(13)
    frames = [rng.randint(0, 256, size=i420_frame_bytes(20, 16)).astype(np.uint8) for _ in range(3)]
    assert len(list(pipeline.upscale_yuv_stream(m, frames, 4, width=20, height=16, depth=2))) == 3


# id -> (run, captures, replays): the graphs the scenario must capture and the replays it must issue
SCENARIOS = {
    "eager-v1": (_train(V1, use_hip_graph=False), 0, 0),
    "eager-v2": (_train(V2, use_hip_graph=False), 0, 0),
    "eager-v1-exits-between-bodies": (_train(V1, use_hip_graph=False, batch_exits=False), 0, 0),
    "eager-v1-no-joint-input-grads": (_train(V1, use_hip_graph=False, joint_input_grads=False), 0, 0),
    "captured-v1-poll": (_train(V1, use_hip_graph=True, early_loss="poll", sync_loss=True), 1, 3),
    "captured-v2-poll": (_train(V2, use_hip_graph=True, early_loss="poll", sync_loss=True), 1, 3),
    "captured-v1-split": (_train(V1, use_hip_graph=True, early_loss="split", sync_loss=True), 2, 6),
    "captured-v2-split": (_train(V2, use_hip_graph=True, early_loss="split", sync_loss=True), 2, 6),
    "captured-v1-late": (_train(V1, use_hip_graph=True, early_loss="poll", sync_loss=True, force_split_backward=True), 2, 6),
    "loader": (_loader_into_step, 1, 3),
    # (a shape is run eagerly at first sight, captured and replayed at the second, replayed from then on; the opaque image
    # of the RGBA stream runs as one batch slot, the others as two)
    "upscale-fp32": (_upscale("fp32"), 1, 4),
    "upscale-fp16": (_upscale("fp16"), 1, 4),
    "upscale-rgba": (_upscale("fp32", keep_alpha=True), 1, 3),
    "upscale-output-size": (_upscale("fp32", output_size=(50, 70)), 1, 4),
    "video": (_video, 1, 2),
}
TRAINING = [k for k in SCENARIOS if k.startswith(("eager", "captured"))]
_RECORDED = {}


def record_scenario(key, monkeypatch, device, strict=True):
    """The scenario's log, recorded once per session: (log, Recorder)."""
    if key not in _RECORDED:
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()    # (the same blocks are handed out whatever ran before: the logs repeat)
        with monkeypatch.context() as mp:
            with SO.Recorder(mp, strict=strict) as rec:
                SCENARIOS[key][0](rec, device)
        torch.cuda.synchronize()
        _RECORDED[key] = (rec.log, rec)
    return _RECORDED[key]


# No exemption has been needed.  An entry is (scenario, {the two launch names}, {the two operand labels}, reason): why the
# pair cannot overlap in time or does not matter.  None may cover a pair that involves a DualChain side stream, the
# LossCopy stream, the pipeline's copy stream or a graph replay (those are what the audit is for), and an entry that
# matches nothing fails the scenario's test.
EXEMPTIONS = []


def _unexempted(key, conflicts):
    used, left = set(), []
    for c in conflicts:
        hit = [i for i, (scenario, names, labels, _) in enumerate(EXEMPTIONS)
               if scenario == key and set(names) == c.names() and set(labels) == c.labels() and c.scope is None
               and not any(n.startswith("replay(") for n in c.names()) and c.streams() <= {0, SO.HOST}]
        used.update(hit)
        if not hit:
            left.append(c)
    stale = [e for i, e in enumerate(EXEMPTIONS) if e[0] == key and i not in used]
    assert not stale, "exemptions that matched nothing: %s" % (stale,)
    return left


def _library_launches(log):
    return [r for r in log if r["kind"] == "access" and r["name"].startswith("larva_")]


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(SCENARIOS))
def test_every_conflicting_pair_of_the_scenario_is_ordered(hip_device, monkeypatch, key):
    """(b) the eager training steps, (c) the captured ones, (d) the device loader into the step's buffers, (e) the
    inference streams: no unordered conflicting pair, inside a capture body or among replays, copies, the LossCopy
    stream, the optimizer launch and the next step's repack, pinned buffers and host accesses included."""
    log, rec = record_scenario(key, monkeypatch, hip_device)
    _, captures, replays = SCENARIOS[key]
    result = SO.audit(log)
    print("%s: %s" % (key, result.summary()))
    assert not rec.missing
    assert len(result.program_streams()) >= 2, "the scenario ran on one stream: %s" % result.summary()
    assert (result.captures, result.replays) == (captures, replays), result.summary()
    assert len(result.pairs) > 0
    if key in TRAINING or key == "loader":
        side = {r["stream"] for i in _edges(log, "join") for r in [_recorded_by(log, i)]}
        assert len(side) == 1, "the half-batch chains never forked"
        assert any(r["stream"] in side and r["name"] == "larva_conv3x3_fwd_strips" for r in _library_launches(log))
        # backward runs on autograd's device thread: the wrappers and the dispatch mode must be there too
        inside = [r for r in _library_launches(log) if r["bw"]]
        assert inside and all(r["mode"] for r in inside), "launches of backward() escaped the recorder"
        assert len({r["thread"] for r in inside} | {log[0]["thread"]}) == 2
    assert set(r["name"] for r in _library_launches(log)) <= set(OPERANDS), "test (a) does not cover an entry point reached here"
    left = _unexempted(key, result.conflicts)
    assert not left, "%d unordered conflicting pairs, the first:\n%s" % (len(left), "\n".join(map(repr, left[:8])))


# ------------------------------------------------------------------------------------------------ (f) the audit bites
# edge class -> (record kind, file, function, which of the site's records in program order: None = all, (k, n) = every
# n-th starting at the k-th)
EDGES = {
    "fork": ("wait", "autograd.py", "conv", None),                     # DualChain.conv: side.wait_stream(main)
    "join": ("wait", "autograd.py", "join", None),                     # DualChain.join: main.wait_stream(side)
    "loss-copy": ("wait", "captured_step.py", "start", None),          # LossCopy.start: stream.wait_event(fwd_done)
    "loss-done": ("host_sync", "captured_step.py", "result", None),    # LossCopy.result: done.synchronize()
    "h2d": ("wait", "pipeline.py", "_stream", None),                   # compute.wait_event(slot.h2d)
    "fwd": ("wait", "pipeline.py", "issue_d2h", None),                 # copy.wait_event(slot.fwd)
    "done": ("host_sync", "pipeline.py", "retire", None),              # slot.done.synchronize()
    "grown": ("wait", "pipeline.py", "_grown", None),                  # copy.wait_stream(compute) for a new device buffer
    "step-warm-up-fork": ("wait", "captured_step.py", "__init__", (0, 2)),
    "step-warm-up-join": ("wait", "captured_step.py", "__init__", (1, 2)),
    "infer-warm-up-fork": ("wait", "inference.py", "_capture_infer", (0, 2)),
    "infer-warm-up-join": ("wait", "inference.py", "_capture_infer", (1, 2)),
}
HALF_BATCH = ("joins at the end of every autograd node: the node's output is next read by another pair of half-batch links, each "
              "of which reads only the images its own stream wrote, so the join behind the head (once per step) orders nothing; "
              "and between the forward nodes the main stream launches nothing that the side chain reads or overwrites (it reads "
              "its own images and the weights packed before the step's first fork, and writes a fresh output), so the forks "
              "behind the first order nothing either.  The lazy joins of the plugin's default step leave exactly these out.")
ONE_CONSUMER = ("without joint input gradients the backward joins per node: the join behind the last exit's chain link and the "
                "fork of the next body's first link have nothing between them that the other stream touches (once per step)")
POOL = ("the wait matters when the allocator hands the slot a block that a forward still in flight has released (the hazard "
        "this audit found in the RGBA stream); where the new buffer's block was idle it orders nothing")
# (scenario, edge class) -> (at most this many edges that nothing reports, why).  An edge that ONE other edge or host sync
# makes redundant needs no entry: the test shows the other (taking both out is reported).  Those are: the wait_stream
# behind a capture's warm-up (torch.cuda.graph synchronises the device before it begins), the first fork of a shape (it
# follows the blocking upload of the strip-tile table), a slot's done.synchronize() when a capture's device
# synchronisation came between its copy and its retirement, and copy.wait_event(slot.fwd) of the image in flight while the
# next slot's buffers are allocated (the copy stream has just waited for the compute stream there).  All of them stay in
# the code: each is load-bearing as soon as the other is not there.
REDUNDANT = {
    ("eager-v1-exits-between-bodies", "fork"): (9, HALF_BATCH), ("eager-v1-exits-between-bodies", "join"): (3, HALF_BATCH),
    ("eager-v1-no-joint-input-grads", "fork"): (3, ONE_CONSUMER), ("eager-v1-no-joint-input-grads", "join"): (3, ONE_CONSUMER),
}
REDUNDANT.update({(k, "grown"): (6, POOL) for k in SCENARIOS if k.startswith(("upscale", "video"))})
BITING = {k: ("fork", "join") for k in TRAINING + ["loader"]}
BITING.update({k: BITING[k] + ("step-warm-up-fork",) for k in SCENARIOS if k.startswith(("captured", "loader"))})
BITING.update({k: BITING[k] + ("loss-copy", "loss-done") for k in SCENARIOS if k.endswith("split")})
BITING.update({k: ("h2d", "fwd", "done", "infer-warm-up-fork") for k in SCENARIOS if k.startswith(("upscale", "video"))})


def _edges(log, cls):
    kind, file, function, which = EDGES[cls]
    found = [i for i in SO.find(log, kind=kind, site=(file, function))]
    return found if which is None else found[which[0]::which[1]]


def _recorded_by(log, i):
    """The `record` whose clock the wait log[i] merges (the last one of its event before it)."""
    return next(log[j] for j in range(i - 1, -1, -1) if log[j]["kind"] == "record" and log[j]["event"] == log[i]["event"])


def _protected(log, i):
    """The two parties the edge log[i] orders: the waiter and the stream the event was recorded on."""
    r = log[i]
    if r["kind"] == "wait":
        return {r["stream"], _recorded_by(log, i)["stream"]}
    return {SO.HOST, _recorded_by(log, i)["stream"] if r.get("event") is not None else r["stream"]}


def _reported_without(log, drop):
    kept = [r for i, r in enumerate(log) if i not in drop]
    return check(kept)


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(BITING))
def test_taking_an_ordering_edge_out_of_the_log_is_reported(hip_device, monkeypatch, key):
    """Every ordering edge of the scenario in turn, removed from the recorded log only (nothing runs): the checker must
    report a pair between exactly the two parties the edge orders.  An edge nothing reports must be shown redundant behind
    ONE other edge or host sync nearby (taking both out is reported between the same two parties: the recorder sees the
    hazard, and something else orders it) or be listed in REDUNDANT."""
    log, _ = record_scenario(key, monkeypatch, hip_device)
    assert check(log) == []
    syncs = SO.find(log, kind="host_sync")
    others = sorted(syncs + SO.find(log, kind="wait"))
    for cls in EDGES:
        edges = _edges(log, cls)
        if cls in BITING[key]:
            assert edges, "the scenario has no %s edge" % cls
        biting, covered, silent = 0, 0, []
        for i in edges:
            found = _reported_without(log, {i})
            if found:
                assert any(c.streams() == _protected(log, i) for c in found), "log[%d] (%s) removed, but the reports are about others: %s" % (i, cls, found[:3])
                biting += 1
                continue
            after = [j for j in syncs if j > i][:3]     # (a split capture synchronises the device once per graph)
            behind = [{j} for j in sorted(others, key=lambda j: abs(j - i))[1:9]] + [set(after[:n]) for n in (2, 3)]
            if any(c.streams() == _protected(log, i) for js in behind for c in _reported_without(log, {i} | js)):
                covered += 1
            else:
                silent.append(i)
        print("%s %s: %d edges, %d load-bearing, %d redundant behind another edge or host sync, %d reported by nothing" % (
            key, cls, len(edges), biting, covered, len(silent)))
        if cls in BITING[key]:
            assert biting > 0, "no %s edge is load-bearing" % cls
        allowed, why = REDUNDANT.get((key, cls), (0, None))
        assert len(silent) <= allowed, "%s edges at log%s: removed, and nothing is reported (redundant, or a hole in the recorder?)" % (cls, silent)
        if cls.endswith("warm-up-join"):
            assert covered == len(edges)


def test_a_new_slot_buffer_first_written_by_the_copy_stream_needs_the_compute_stream():
    """What the audit found in pipeline._Slot._grown, as a log: image 0's eager forward releases an activation while it is
    still in flight on the compute stream, the second slot's new device input buffer is carved out of that block (it is
    the compute stream's allocation), and image 1's host-to-device copy is the first to write it, on the copy stream."""
    forward = [access(MAIN, "conv", reads=buf(B, "src"), writes=buf(A, "out")), access(MAIN, "conv", reads=buf(A, "src"), writes=buf(C, "out"))]
    h2d = [host_access(writes=buf(0x9000, "pin.in")), access(COPY, "copy_", reads=buf(0x9000, "src"), writes=buf(A, "self", 0, 0x40))]
    found = check(forward + h2d)
    assert [c.kind() for c in found] == ["WaW", "WaR"] and all(c.streams() == {MAIN, COPY} for c in found)
    assert check(forward + [SO.record_stream(A, A + 0x40, COPY)] + wait_stream(COPY, MAIN, "grown") + h2d) == []


# ------------------------------------------------------------------------------------------------ (a) footprints
def _f32(device, *shape):
    return torch.rand(*shape, device=device)


def _u8(device, *shape):
    return torch.randint(0, 256, shape, dtype=torch.uint8, device=device)


def _whole(t):
    """The allocation behind a result the wrapper hands back as a prefix view (partial sums)."""
    return t if t._base is None else t._base


def _pack_jobs(K, dev):
    w, w3 = _f32(dev, 48, 48, 3, 3), _f32(dev, 48, 3, 3, 3)
    new = lambda a, b: torch.empty(K.packed_weight_floats(a, b), device=dev)
    jobs = [(w, new(48, 48), new(48, 48), 48, 48, 0), (w3, new(48, 16), None, 48, 16, 0)]
    return jobs, {"w[0]": w, "w[1]": w3, "wpk_fwd[0]": jobs[0][1], "wpk_bwd[0]": jobs[0][2], "wpk_fwd[1]": jobs[1][1]}


def _act(dev, c=48):
    return _f32(dev, 5, c, 16, 20)


def _wpk(K, dev, cout=48, cin=48):
    return torch.rand(K.packed_weight_floats(cout, cin), device=dev)


def _op_pack(K, dev):
    jobs, want = _pack_jobs(K, dev)
    K.pack_weights_batch(jobs)
    return want


def _op_prologue(K, dev):
    jobs, want = _pack_jobs(K, dev)
    x, x16, base = _f32(dev, 5, 3, 16, 20), torch.zeros(5, 16, 16, 20, device=dev), torch.empty(5, 3, 64, 80, device=dev)
    K.step_prologue(jobs, x, x16, base)
    return dict(want, x=x, x16=x16, base=base)


def _op_pitched(K, dev):
    s0, s1, r0, r1, wpk, bias = _act(dev), _act(dev), _act(dev), _act(dev), _wpk(K, dev, 48, 96), _f32(dev, 48)
    out = torch.empty(5, 48, 16, 20, device=dev)
    K.conv3x3([s0, s1], wpk, 48, bias=bias, res0=r0, res1=r1, out=out, images=(1, 4))
    return {"src[0]": s0[1:4], "src[1]": s1[1:4], "wpk": wpk, "bias": bias, "res0": r0[1:4], "res1": r1[1:4], "out": out[1:4]}


def _op_strips(K, dev):
    s, m, wpk, bias = _act(dev), _act(dev), _wpk(K, dev), _f32(dev, 48)
    out = torch.empty(5, 48, 16, 20, device=dev)
    K.conv3x3(s, wpk, 48, bias=bias, mask=m, out=out, images=(2, 5), strips=2, plain_stores=True)
    return {"src[0]": s[2:5], "wpk": wpk, "bias": bias, "mask": m[2:5], "out": out[2:5], "tile_tab": K.strip_tile_table(16, 20, dev, phase=1)[0]}


def _op_batch(K, dev):
    jobs = [{"srcs": _act(dev), "wpk": _wpk(K, dev), "bias": _f32(dev, 48), "base": _f32(dev, 5, 3, 64, 80)} for _ in range(2)]
    outs = K.conv3x3_batch(jobs, 48, shuffle=True)
    want = {"out[%d]" % i: o for i, o in enumerate(outs)}
    for i, j in enumerate(jobs):
        want.update({"src[%d]" % i: j["srcs"], "wpk[%d]" % i: j["wpk"], "bias[%d]" % i: j["bias"], "base[%d]" % i: j["base"]})
    return want


def _op_exit_l1(K, dev):
    jobs = [{"srcs": _act(dev), "wpk": _wpk(K, dev), "bias": _f32(dev, 48), "base": _f32(dev, 5, 3, 64, 80)} for _ in range(2)]
    truth = _f32(dev, 5, 3, 64, 80)
    outs, parts, grads = K.conv3x3_exit_l1_batch(jobs, 48, truth, 1.0, 0.5, [False, True])
    want = {"truth[0]": truth, "truth[1]": truth, "out[1]": outs[1]}
    for i, j in enumerate(jobs):
        want.update({"src[%d]" % i: j["srcs"], "wpk[%d]" % i: j["wpk"], "bias[%d]" % i: j["bias"], "base[%d]" % i: j["base"],
                     "grad[%d]" % i: grads[i], "partial[%d]" % i: parts[i]})
    return want


def _wgrad_jobs(dev, n=2):
    return [{"dy": _act(dev), "x": _act(dev)} for _ in range(n)]


def _op_wgrad_partial(K, dev):
    jobs = _wgrad_jobs(dev)
    parts, _ = K.conv3x3_wgrad_partial(jobs, 48, 48, 8)
    want = {"partial[%d]" % i: p for i, p in enumerate(parts)}
    for i, j in enumerate(jobs):
        want.update({"dy[%d]" % i: j["dy"], "x[%d]" % i: j["x"]})
    return want


def _op_wgrad_flat(K, dev, head=False):
    jobs = _wgrad_jobs(dev)
    extra = {"dy": _act(dev), "x": _act(dev, 16)} if head else None
    parts, _ = K.conv3x3_wgrad_partial_flat(jobs, 48, 48, 256, head=extra)
    want = {"partial[%d]" % i: _whole(p) for i, p in enumerate(parts[:2])}
    for i, j in enumerate(jobs):
        want.update({"dy[%d]" % i: j["dy"], "x[%d]" % i: j["x"]})
    if head:
        want.update({"head_dy": extra["dy"], "head_x16": extra["x"], "head_partial": _whole(parts[2])})
    return want


def _op_reduce(K, dev, loss=False):
    parts, used = K.conv3x3_wgrad_partial(_wgrad_jobs(dev), 48, 48, 8)
    jobs = [{"partial": p, "splits": used, "dw": torch.empty(48, 48, 3, 3, device=dev), "db": torch.empty(48, device=dev)} for p in parts]
    want = {}
    for i, j in enumerate(jobs):
        want.update({"partial[%d]" % i: j["partial"], "dw[%d]" % i: j["dw"], "db[%d]" % i: j["db"]})
    if loss:
        terms, out = [_f32(dev, 7), _f32(dev, 1)[0].clone()], torch.empty((), device=dev)
        K.wgrad_reduce(jobs, 48, 48, loss=(terms, [0.5, 1.0], 2.0, out))
        want.update({"terms[0]": terms[0], "terms[1]": terms[1], "loss_out": out})
    else:
        K.wgrad_reduce(jobs, 48, 48)
    return want


def _op_loss(K, dev):
    cell, terms = K.HostCell(), [_f32(dev, 7), _f32(dev, 3)]
    out = K.loss_from_partials(terms, [1.0, 1.0], 2.0, host_cell=cell)
    torch.cuda.synchronize()
    return {"terms[0]": terms[0], "terms[1]": terms[1], "out": out, "host_cell": (cell.ptr, 8), "dev_seq": cell.dev_seq}


def _op_l1_fwd(K, dev):
    a, b = _f32(dev, 5, 3, 64, 80), _f32(dev, 5, 3, 64, 80)
    return {"a": a, "b": b, "loss": K.l1_fwd(a, b), "partial": K._l1_workspace(dev)}


def _op_l1_bwd(K, dev):
    a, b, g = _f32(dev, 5, 3, 64, 80), _f32(dev, 5, 3, 64, 80), torch.ones((), device=dev)
    return {"a": a, "b": b, "gout": g, "ga": K.l1_bwd(a, b, g)}


def _op_l1_partial_grad(K, dev):
    a, b = _f32(dev, 5, 3, 64, 80), _f32(dev, 5, 3, 64, 80)
    part, _, grad = K.l1_partial_grad(a, b, 1.0, 0.5)
    return {"a": a, "b": b, "partial": _whole(part), "grad": grad}


def _op_unshuffle(K, dev):
    g = _f32(dev, 5, 3, 64, 80)
    return {"in": g, "out": K.pixel_unshuffle4(g)}


def _op_upsample(K, dev):
    x = _f32(dev, 5, 3, 16, 20)
    return {"in": x, "out": K.upsample4(x)}


def _op_adamw(K, dev):
    p, g, m, v = (_f32(dev, 1003) for _ in range(4))
    K.adamw_step_host(p, g, m, v, 1, 1e-3, 0.9, 0.999, 1e-8, 0.01)
    return {"p": p, "g": g, "m": m, "v": v}


def _op_gather(K, dev):
    data = _u8(dev, 2 * 3 * 24 * 24)
    offsets, hw = torch.tensor([0, 3 * 24 * 24]).to(dev), torch.tensor([24, 24, 24, 24], dtype=torch.int32).to(dev)
    draws = torch.tensor([[0, 1, 2, 0, 0], [1, 0, 0, 1, 1]], dtype=torch.int32).to(dev)
    return {"data": data, "offsets": offsets, "hw": hw, "draws": draws, "out": K.gather_patches(data, offsets, hw, draws, 2, 8, 1)}


def _op_u8_in(K, dev):
    x = _u8(dev, 2, 16, 20, 3)
    return {"in": x, "out": K.u8_hwc_to_f32_chw(x)}


def _op_u8_out(K, dev):
    x = _f32(dev, 2, 3, 16, 20)
    return {"in": x, "out": K.f32_chw_to_u8_hwc(x)}


def _op_f16_pack(K, dev):
    w = _f32(dev, 48, 96, 3, 3)
    return {"w": w, "wpk": K.f16_pack_weights(w)}


def _flag(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def _op_f16_head(K, dev):
    x, w, bias, flag = _f32(dev, 2, 3, 16, 20), _f32(dev, 48, 3, 3, 3), _f32(dev, 48), _flag(dev)
    return {"x": x, "w": w, "bias": bias, "flag": flag, "out": K.f16_head(x, w, bias, flag)}


def _half_act(dev):
    return torch.rand(2, 16, 20, 48, device=dev).half()


def _op_f16_conv(K, dev):
    s0, s1, r0, r1, bias, flag = _half_act(dev), _half_act(dev), _half_act(dev), _half_act(dev), _f32(dev, 48), _flag(dev)
    wpk = K.f16_pack_weights(_f32(dev, 48, 96, 3, 3) * 0.01)
    return {"srcs[0]": s0, "srcs[1]": s1, "wpk": wpk, "bias": bias, "res0": r0, "res1": r1, "flag": flag,
            "out": K.f16_conv3x3([s0, s1], wpk, bias, flag, res0=r0, res1=r1)}


def _op_f16_leg_end(K, dev):
    src, bias, base, flag = _half_act(dev), _f32(dev, 48), _f32(dev, 2, 3, 64, 80), _flag(dev)
    wpk = K.f16_pack_weights(_f32(dev, 48, 48, 3, 3) * 0.01)
    return {"src": src, "wpk": wpk, "bias": bias, "base": base, "flag": flag, "out": K.f16_conv3x3_shuffle_base_u8(src, wpk, bias, base, flag)}


def _op_rgba_split(K, dev):
    x, slot = _u8(dev, 2, 16, 20, 4), torch.tensor([2, -1], dtype=torch.int32).to(dev)
    return {"rgba": x, "alpha_slot": slot, "out": K.rgba_u8_split_f32(x, slot, 1)}


def _op_rgba_merge(K, dev):
    rgb, slot = _u8(dev, 3, 64, 80, 3), torch.tensor([2, -1], dtype=torch.int32).to(dev)
    return {"rgb": rgb, "alpha_slot": slot, "out": K.rgb_u8_merge_rgba(rgb, slot, 2)}


def _op_resize(K, dev):
    x = _u8(dev, 2, 64, 80, 3)
    out = K.resize_u8(x, 50, 70)
    (hb, hc, _), (vb, vc, _) = K._resize_tables(80, 70, dev), K._resize_tables(64, 50, dev)
    return {"src": x, "dst": out, "hbounds": hb, "hcoeffs": hc, "vbounds": vb, "vcoeffs": vc}


def _op_i420_in(K, dev):
    frames = _u8(dev, 2, 480)
    return {"frames": frames, "out": K.i420_to_rgb_f32(frames, 20, 16)}


def _op_i420_out(K, dev):
    x = _u8(dev, 2, 16, 20, 3)
    return {"img": x, "out": K.rgb_u8_to_i420(x)}


# entry point -> its kernels.py wrapper called once on fresh tensors of exactly the operand shapes (with an images=
# sub-range where the wrapper has one) -> {operand label: the tensor (or view) the launch must have been recorded with}
OPERANDS = {
    "larva_pack_weights_batch": _op_pack, "larva_step_prologue": _op_prologue, "larva_conv3x3_fwd_pitched": _op_pitched,
    "larva_conv3x3_fwd_strips": _op_strips, "larva_conv3x3_fwd_batch": _op_batch, "larva_conv3x3_exit_l1_batch": _op_exit_l1,
    "larva_conv3x3_wgrad_partial": _op_wgrad_partial, "larva_conv3x3_wgrad_partial_flat": _op_wgrad_flat,
    "larva_conv3x3_wgrad_partial_flat_head": lambda K, dev: _op_wgrad_flat(K, dev, head=True),
    "larva_wgrad_reduce": _op_reduce, "larva_wgrad_reduce_with_loss": lambda K, dev: _op_reduce(K, dev, loss=True),
    "larva_loss_from_partials_to_host_seq": _op_loss, "larva_l1_fwd": _op_l1_fwd, "larva_l1_bwd": _op_l1_bwd,
    "larva_l1_partial_grad": _op_l1_partial_grad, "larva_pixel_unshuffle4": _op_unshuffle, "larva_upsample4_fwd": _op_upsample,
    "larva_adamw_step_host": _op_adamw, "larva_gather_patches": _op_gather, "larva_u8_hwc_to_f32_chw": _op_u8_in,
    "larva_f32_chw_to_u8_hwc": _op_u8_out, "larva_f16_pack_weights": _op_f16_pack, "larva_f16_head": _op_f16_head,
    "larva_f16_conv3x3": _op_f16_conv, "larva_f16_conv3x3_shuffle_base_u8": _op_f16_leg_end,
    "larva_rgba_u8_split_f32": _op_rgba_split, "larva_rgb_u8_merge_rgba": _op_rgba_merge, "larva_resize_u8": _op_resize,
    "larva_i420_to_rgb_f32": _op_i420_in, "larva_rgb_u8_to_i420": _op_i420_out,
}


def test_every_declared_footprint_is_exercised():
    assert set(OPERANDS) == set(SO.FOOTPRINTS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(OPERANDS))
def test_the_recorded_footprint_is_the_operand(hip_device, monkeypatch, name):
    """Each pointer operand's recorded range starts at the tensor's data_ptr() (the sub-range's first image) and is as
    long as the tensor (the sub-range): a too-small extent would hide a conflict, a too-large one invent one."""
    from larvanet_amd import hip_lib, kernels as K
    with monkeypatch.context() as mp:
        with SO.Recorder(mp) as rec:
            want = OPERANDS[name](K, hip_device)
    torch.cuda.synchronize()
    launches = [r for r in rec.log if r["kind"] == "access" and r["name"] == name]
    assert launches, "the wrapper did not reach %s" % name
    r = launches[-1]
    const = {p.name: p.const for p in SO.parse_params(hip_lib.HEADER_PATH)[name]}
    got = {label: (lo, hi - lo, "r") for lo, hi, label in r["reads"]}
    got.update({label: (lo, hi - lo, "w") for lo, hi, label in r["writes"]})
    expect = {}
    for label, t in want.items():
        ptr, nbytes = t if isinstance(t, tuple) else (t.data_ptr(), t.numel() * t.element_size())
        assert isinstance(t, tuple) or t.is_contiguous(), label
        expect[label] = (ptr, nbytes, "r" if const[label.split("[")[0]] else "w")
    assert got == expect
    assert r["stream"] == torch.cuda.current_stream().cuda_stream
