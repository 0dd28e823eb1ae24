"""Cross-stream launch order, audited on the host (helper of tests/test_stream_order.py, imported by path).

A value test cannot see a missing wait: the racing launch nearly always finishes first at the test shapes.  This helper
records WHAT a scenario launches (library entry points, torch's own device work, graph captures and replays), on WHICH
stream, over WHICH bytes, and every ordering edge between streams, as a plain list of records (a "log", JSON-able), and
`check(log)` proves with vector clocks that every conflicting pair of accesses is ordered.  Nothing racy is ever run:
defects are seeded into a recorded log (drop_record), never into the program.

The model
  * Same stream = ordered.  `record(event, stream)` snapshots the stream's clock, `wait(stream, event)` merges that
    snapshot into the waiting stream (a.wait_stream(b) = a record on b plus a wait on a).  A wait on an event recorded
    BEFORE the launch it is meant to cover therefore orders nothing.
  * Streams do not order each other implicitly.  torch's streams are created non-blocking (hipStreamNonBlocking), so the
    null stream gives no order either: the legacy "the default stream waits for everybody" rule does not apply to them,
    and the checker treats stream 0 as one more stream.
  * A host sync (stream / event / device) orders everything the host issues LATER, on any stream, after what it waited for.
  * Two accesses conflict when their byte ranges overlap and at least one writes.  A `host_access` (the host touching
    pinned memory) conflicts with every earlier device access to those bytes that the host has not waited for; device
    work issued after it is ordered behind it (the host had finished).
  * Records between capture_begin and capture_end are the graph's BODY: they do not run, so they conflict with nothing
    outside; inside the body the same rules hold, on clocks of its own.  A `replay` is ONE access on the replaying stream
    whose reads and writes are the union of the body's.  Graphs of one memory pool are not special: their buffers
    overlap by address, which is the point.
  * What the log does not contain.  (1) The caching allocator hands a block that was `record_stream`ed to another stream
    back only after it has seen that stream's event complete; (2) a block freed WITHOUT record_stream is reused at once,
    but only by an allocation on the stream it was allocated on, i.e. behind everything that stream was made to wait for;
    (3) hipMalloc / hipFree and empty_cache synchronise the device.  (2) and (3) need no modelling: a reuse the log sees
    is a later access on the allocating stream and is checked like any other -- that is exactly how a tensor dropped
    from DualChain._keep would show.  (1) is modelled, not waived: `record_stream` records are kept in the log, and the
    first access to a recorded range AFTER its tensor died (the recorder logs `free` from a weak reference) is ordered
    behind the recorded stream's accesses up to the free, which is what the allocator's event guarantees (the tensor
    object that was recorded is taken to own its memory).  No scenario of the suite has needed the rule so far (the
    pipeline's slots outlive their generator's last host wait); it is exercised by a hand-written log.

The recorder (Recorder) is built on pytest's monkeypatch only: wrappers on every larva_* launch of the object
hip_lib.load() returns (kernels._launch looks the entry point up per call), a TorchDispatchMode for torch's own device
work, patches of the Python-level ordering calls of torch.cuda, and wrappers on the pipeline's host side.
"""
import bisect
import ctypes
import os
import re
import sys
import threading
import weakref

HOST = "host"


# ------------------------------------------------------------------------------------------------ the log's records
def access(stream, name, reads=(), writes=(), **meta):
    """One launch on `stream`; reads / writes: [(lo, hi, label)] byte ranges [lo, hi)."""
    return dict(meta, kind="access", stream=stream, name=name, reads=[list(r) for r in reads], writes=[list(w) for w in writes])


def record(event, stream, **meta):
    return dict(meta, kind="record", event=event, stream=stream)


def wait(stream, event, **meta):
    return dict(meta, kind="wait", stream=stream, event=event)


def wait_stream(waiter, other, token):
    """a.wait_stream(b): two records."""
    return [record(token, other, origin="wait_stream"), wait(waiter, token, origin="wait_stream")]


def host_sync(stream=None, event=None, **meta):
    """The host waits for a stream, an event, or (neither given) the device."""
    return dict(meta, kind="host_sync", stream=stream, event=event)


def host_access(reads=(), writes=(), name="host", **meta):
    """The host itself touches pinned memory."""
    return dict(meta, kind="host_access", name=name, reads=[list(r) for r in reads], writes=[list(w) for w in writes])


def capture_begin(graph, stream, **meta):
    return dict(meta, kind="capture_begin", graph=graph, stream=stream)


def capture_end(graph, **meta):
    return dict(meta, kind="capture_end", graph=graph)


def replay(graph, stream, **meta):
    return dict(meta, kind="replay", graph=graph, stream=stream)


def record_stream(lo, hi, stream, **meta):
    return dict(meta, kind="record_stream", lo=lo, hi=hi, stream=stream)


def free(lo, hi, **meta):
    return dict(meta, kind="free", lo=lo, hi=hi)


def drop_record(log, index):
    """The log without record `index`: how a defect is seeded (an ordering edge that was never issued)."""
    return log[:index] + log[index + 1:]


# ------------------------------------------------------------------------------------------------ the checker
class Conflict:
    """An unordered conflicting pair.  first / second: dicts {name, stream, label, index, write}; [lo, hi) the overlap;
    scope: None = the program, else the graph whose body holds the pair."""

    def __init__(self, scope, first, second, lo, hi):
        self.scope, self.first, self.second, self.lo, self.hi = scope, first, second, lo, hi

    def streams(self):
        return {self.first["stream"], self.second["stream"]}

    def names(self):
        return {self.first["name"], self.second["name"]}

    def labels(self):
        return {self.first["label"], self.second["label"]}

    def kind(self):
        """RaW / WaR / WaW: the later access after the earlier one."""
        return ("W" if self.second["write"] else "R") + "a" + ("W" if self.first["write"] else "R")

    def __repr__(self):
        def side(s):
            return "%s %s.%s on stream %s (log[%d])" % ("write" if s["write"] else "read", s["name"], s["label"],
                                                        _hex(s["stream"]), s["index"])
        where = "" if self.scope is None else " inside graph %s" % (self.scope,)
        return "unordered%s: %s <-> %s over [%#x, %#x) (%d bytes)" % (where, side(self.first), side(self.second), self.lo,
                                                                     self.hi, self.hi - self.lo)


def _hex(s):
    return "%#x" % s if isinstance(s, int) else str(s)


class _Acc:
    __slots__ = ("index", "stream", "tick", "name", "label", "write")

    def __init__(self, index, stream, tick, name, label, write):
        self.index, self.stream, self.tick, self.name, self.label, self.write = index, stream, tick, name, label, write

    def side(self):
        return {"name": self.name, "stream": self.stream, "label": self.label, "index": self.index, "write": self.write}


class _Seg:
    __slots__ = ("write", "reads", "guard")

    def __init__(self, write=None, reads=None, guard=None):
        self.write, self.reads, self.guard = write, reads or {}, guard

    def copy(self):
        return _Seg(self.write, dict(self.reads), self.guard)


def _merge(into, other):
    for k, v in other.items():
        if into.get(k, 0) < v:
            into[k] = v


class _Space:
    """Clocks and shadow memory of the program, or of one capture body."""

    def __init__(self, scope, result):
        self.scope, self.result = scope, result
        self.clock, self.events, self.host = {}, {}, {}
        self.bounds, self.segs = [0], [_Seg()]     # segment i covers [bounds[i], bounds[i + 1])
        self.found = {}
        self.recorded = []                         # record_stream: [lo, hi, stream]
        self.reads, self.writes = {}, {}           # a body's union: (lo, hi) -> label

    def _split(self, x):
        i = bisect.bisect_right(self.bounds, x) - 1
        if self.bounds[i] != x:
            self.bounds.insert(i + 1, x)
            self.segs.insert(i + 1, self.segs[i].copy())
            i += 1
        return i

    def _range(self, lo, hi):
        i, j = self._split(lo), self._split(hi)
        return range(i, j)

    def _now(self, stream):
        vc = self.clock.setdefault(stream, {})
        _merge(vc, self.host)
        return vc

    def _report(self, prev, acc, lo, hi):
        key = (prev.index, acc.index, prev.label, acc.label, prev.write, acc.write)
        c = self.found.get(key)
        if c is None:
            self.found[key] = Conflict(self.scope, prev.side(), acc.side(), lo, hi)
        else:
            c.lo, c.hi = min(c.lo, lo), max(c.hi, hi)

    def _against(self, prev, acc, vc, lo, hi):
        """prev (earlier) against acc (now, clock vc); acc on HOST: vc is what the host has waited for."""
        if prev is None or prev.stream == acc.stream or prev.stream == HOST:
            return
        self.result.pairs.add((self.scope, prev.index, acc.index))
        if vc.get(prev.stream, 0) < prev.tick:
            self._report(prev, acc, lo, hi)

    def launch(self, index, stream, name, reads, writes):
        host = stream == HOST
        if host:
            vc, tick = self.host, 0
        else:
            vc = self._now(stream)
            vc[stream] = tick = vc.get(stream, 0) + 1
            self.result.launches += 1
            self.result.streams.add((self.scope, stream))
        touched = []
        for ops, is_write in ((reads, False), (writes, True)):
            for lo, hi, label in ops:
                if hi <= lo:
                    continue
                acc = _Acc(index, stream, tick, name, label, is_write)
                for i in self._range(lo, hi):
                    seg = self.segs[i]
                    a, b = max(lo, self.bounds[i]), min(hi, self.bounds[i + 1]) if i + 1 < len(self.bounds) else hi
                    if seg.guard is not None:     # first touch after a record_stream'ed tensor died: the allocator's event
                        _merge(vc, seg.guard)
                        seg.guard = None
                    self._against(seg.write, acc, vc, a, b)
                    if is_write:
                        for r in seg.reads.values():
                            self._against(r, acc, vc, a, b)
                    touched.append((seg, acc))
                if self.scope is not None:
                    (self.writes if is_write else self.reads).setdefault((lo, hi), "%s.%s" % (name, label))
        for seg, acc in touched:   # (after all checks: a launch does not conflict with itself)
            if acc.write:
                seg.write, seg.reads = acc, {}
            elif not host:
                seg.reads[stream] = acc

    def record_event(self, event, stream):
        self.events[event] = dict(self._now(stream))

    def wait_event(self, stream, event):
        _merge(self._now(stream), self.events.get(event, {}))

    def sync(self, stream, event):
        if event is not None:
            _merge(self.host, self.events.get(event, {}))
        elif stream is not None:
            _merge(self.host, self.clock.get(stream, {}))
        else:
            for vc in self.clock.values():
                _merge(self.host, vc)

    def freed(self, lo, hi):
        for rlo, rhi, stream in self.recorded:
            if rlo < hi and lo < rhi:
                for i in self._range(max(lo, rlo), min(hi, rhi)):
                    seg = self.segs[i]
                    seg.guard = dict(seg.guard or {})
                    _merge(seg.guard, self.clock.get(stream, {}))
        self.recorded = [r for r in self.recorded if not (r[0] < hi and lo < r[1])]


class Audit:
    """check()'s working: conflicts, and how much was looked at."""

    def __init__(self):
        self.conflicts, self.pairs, self.streams = [], set(), set()
        self.launches = self.captures = self.replays = 0

    def program_streams(self):
        return {s for scope, s in self.streams if scope is None}

    def summary(self):
        return "%d launches, %d streams, %d captures, %d replays, %d cross-stream conflicting pairs checked, %d unordered" % (
            self.launches, len(self.program_streams()), self.captures, self.replays, len(self.pairs), len(self.conflicts))


def audit(log):
    result = Audit()
    program = _Space(None, result)
    body, body_graph, graphs = None, None, {}
    for index, r in enumerate(log):
        kind = r["kind"]
        space = body if body is not None else program
        if kind == "access":
            space.launch(index, r["stream"], r["name"], r["reads"], r["writes"])
        elif kind == "host_access":   # the host acts now, whatever is being captured
            program.launch(index, HOST, r.get("name", "host"), r["reads"], r["writes"])
        elif kind == "record":
            space.record_event(r["event"], r["stream"])
        elif kind == "wait":
            space.wait_event(r["stream"], r["event"])
        elif kind == "host_sync":
            if body is not None:
                raise ValueError("log[%d]: the host waits inside the capture of graph %s" % (index, body_graph))
            program.sync(r.get("stream"), r.get("event"))
        elif kind == "capture_begin":
            if body is not None:
                raise ValueError("log[%d]: capture of %s begins inside the capture of %s" % (index, r["graph"], body_graph))
            body, body_graph = _Space(r["graph"], result), r["graph"]
            body._now(r["stream"])
            result.captures += 1
        elif kind == "capture_end":
            if body is None or r["graph"] != body_graph:
                raise ValueError("log[%d]: capture_end of %s without its capture_begin" % (index, r["graph"]))
            graphs[body_graph] = ([(lo, hi, label) for (lo, hi), label in body.reads.items()],
                                  [(lo, hi, label) for (lo, hi), label in body.writes.items()])
            result.conflicts += list(body.found.values())
            body = body_graph = None
        elif kind == "replay":
            if body is not None:
                raise ValueError("log[%d]: replay inside a capture" % index)
            if r["graph"] not in graphs:
                raise ValueError("log[%d]: replay of graph %s, which was never captured" % (index, r["graph"]))
            reads, writes = graphs[r["graph"]]
            program.launch(index, r["stream"], "replay(%s)" % (r["graph"],), reads, writes)
            result.replays += 1
        elif kind == "record_stream":
            space.recorded.append([r["lo"], r["hi"], r["stream"]])
        elif kind == "free":
            program.freed(r["lo"], r["hi"])
        elif kind != "note":
            raise ValueError("log[%d]: unknown record kind %r" % (index, kind))
    if body is not None:
        raise ValueError("the capture of graph %s never ends" % (body_graph,))
    result.conflicts += list(program.found.values())
    result.conflicts.sort(key=lambda c: (c.second["index"], c.first["index"]))
    return result


def check(log):
    """-> the unordered conflicting pairs of the log ([] = every conflicting pair is ordered)."""
    return audit(log).conflicts


# ------------------------------------------------------------------------------------------------ the header
class Param:
    __slots__ = ("name", "pointer", "const", "stream")

    def __init__(self, name, pointer, const, stream):
        self.name, self.pointer, self.const, self.stream = name, pointer, const, stream


def parse_params(path):
    """entry point -> [Param] of every `ret larva_name(args);` of the C header: parameter names and the const-ness of
    what a pointer points to (`const T*` / `const T* const*` = read, `T*` / `T* const*` = written), which
    hip_lib.parse_header drops."""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    text = re.sub(r"//[^\n]*|^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r"\btypedef\s+struct\b[^{;]*\{.*?\}[^;]*;", " ", text, flags=re.S)
    text = re.sub(r'\bextern\s+"C"\s*\{|\}', " ", text)
    out = {}
    for decl in (" ".join(d.split()) for d in text.split(";")):
        m = re.fullmatch(r"(.+?)\b(larva_\w+) ?\((.*)\)", decl) if decl else None
        if m is None:
            continue
        params = []
        for a in ([] if m.group(3).strip() in ("", "void") else m.group(3).split(",")):
            words = re.sub(r"\bconst\b|\*", " ", a).split()
            pointer = "*" in a
            params.append(Param(words[-1], pointer, a.strip().startswith("const"),
                                pointer and words[-1] == "stream" and words[0] == "void"))
        out[m.group(2)] = params
    return out


def is_launch(params):
    """An entry point that launches takes the stream as its last argument; the others (sizes, tables, the host cell) are
    host functions and are not recorded."""
    return bool(params) and params[-1].stream


# ------------------------------------------------------------------------------------------------ footprints
# entry point -> {"dev": {pointer parameter: bytes(a)}, "host": (pointer parameters that are host arrays / results)}.
# `a` holds the call's arguments by parameter name (host arrays as lists); bytes(a) is the extent of the operand -- one
# int for every element of a pointer array, or a list with one int per element -- taken from the shapes include/larva_hip.h
# documents.  A half-batch launch offsets the pointers and passes its image count as N, so the extents follow N.
# TENSOR: a table whose size no scalar argument states (the resident dataset): the extent is that of the torch tensor
# that starts at the pointer, which the recorder has seen being made.
TENSOR = "tensor"
F32, F16 = 4, 2


def _stride(c):
    return c if c % 32 in (0, 16) else c + 16


def packed_weight_bytes(cout, cin):
    return F32 * (cin // 8) * 9 * 8 * _stride(cout)


def _lib():
    from larvanet_amd import hip_lib
    return hip_lib.load()


def _f16_packed(m):
    return F16 * m * 14 * 3 * 64 * 8


def _conv_ops(pitch, src="src"):
    def lr(a):
        return F32 * a.N * a.cout * a.H * pitch(a)

    def hr(a):
        return F32 * a.N * a.cout * a.H * a.W     # [N][cout / 16][4 H][4 W]
    return {src: lambda a: F32 * a.N * a.cin_per_src * a.H * pitch(a),
            "wpk": lambda a: packed_weight_bytes(a.cout, a.n_src * a.cin_per_src), "bias": lambda a: F32 * a.cout,
            "res0": lr, "res1": lr, "mask": lr, "base": hr, "out": lambda a: hr(a) if a.mode else lr(a)}


_PITCHED = _conv_ops(lambda a: a.pitch)
_PACK = {"w": lambda a: [F32 * co * tot * 9 for co, tot in zip(a.cout, a.w_cin_total)],
         "wpk_fwd": lambda a: [packed_weight_bytes(co, ci) for co, ci in zip(a.cout, a.cin)],
         "wpk_bwd": lambda a: [packed_weight_bytes(ci, co) for co, ci in zip(a.cout, a.cin)]}
_PACK_HOST = ("cout", "cin", "w_cin_total", "w_cin_off")


def _tiles(a):
    return a.N * ((a.H + 2) // 3) * ((a.W + 47) // 48)


def _wgrad_partial(a, cout, cin, splits):
    return F32 * int(_lib().larva_wgrad_partial_floats(cout, cin, splits))


_REDUCE = {"partial": lambda a: [_wgrad_partial(a, co, ci, s) for co, ci, s in zip(a.cout, a.cin, a.splits)],
           "dw": lambda a: [F32 * co * tot * 9 for co, tot in zip(a.cout, a.w_cin_total)],
           "db": lambda a: [F32 * co for co in a.cout]}
_REDUCE_HOST = ("cin_off", "cin_valid", "w_cin_total", "splits", "cout", "cin")
_ADAMW = {k: (lambda a: F32 * a.n) for k in "pgmv"}


def _l1_ws(a):
    return F32 * int(_lib().larva_l1_workspace_floats())


def _i420_bytes(a):
    return (a.N - 1) * a.frame_pitch_bytes + a.H * a.W + 2 * ((a.H + 1) // 2) * ((a.W + 1) // 2)


def _f16_act(a):
    return F16 * a.N * a.H * a.W * 48


def _hr3(a):
    return F32 * a.N * 3 * 16 * a.H * a.W


FOOTPRINTS = {
    "larva_pack_weights_batch": {"dev": dict(_PACK), "host": _PACK_HOST},
    "larva_step_prologue": {"dev": dict(_PACK, x=lambda a: F32 * a.N * a.C * a.H * a.W, x16=lambda a: F32 * a.N * 16 * a.H * a.W,
                                        base=lambda a: F32 * a.N * a.C * 16 * a.H * a.W), "host": _PACK_HOST},
    "larva_conv3x3_fwd_pitched": {"dev": dict(_PITCHED), "host": ()},
    "larva_conv3x3_fwd_strips": {"dev": dict(_PITCHED, tile_tab=lambda a: 4 * a.tiles_per_image), "host": ("tile_tab_host",)},
    "larva_conv3x3_fwd_batch": {"dev": dict(_PITCHED), "host": ()},
    "larva_conv3x3_exit_l1_batch": {
        "dev": {"src": lambda a: F32 * a.N * a.cin_per_src * a.H * a.pitch,
                "wpk": lambda a: packed_weight_bytes(a.cout, a.n_src * a.cin_per_src), "bias": lambda a: F32 * a.cout,
                "base": lambda a: F32 * a.N * a.cout * a.H * a.W, "truth": lambda a: F32 * a.N * a.cout * a.H * a.W,
                "out": lambda a: F32 * a.N * a.cout * a.H * a.W, "grad": lambda a: F32 * a.N * a.cout * a.H * a.pitch,
                "partial": lambda a: F32 * int(_lib().larva_exit_l1_partials(a.N, a.H, a.pitch))}, "host": ()},
    "larva_conv3x3_wgrad_partial_flat": {
        "dev": {"dy": lambda a: F32 * a.N * a.cout * a.H * a.W, "x": lambda a: F32 * a.N * a.cin * a.H * a.W,
                "partial": lambda a: _wgrad_partial(a, a.cout, a.cin, int(_lib().larva_wgrad_flat_max_splits(a.njobs, a.nwg, _tiles(a))))},
        "host": ("splits_out",)},
    "larva_conv3x3_wgrad_partial_flat_head": {
        "dev": {"dy": lambda a: F32 * a.N * 48 * a.H * a.W, "x": lambda a: F32 * a.N * 48 * a.H * a.W,
                "partial": lambda a: _wgrad_partial(a, 48, 48, int(_lib().larva_wgrad_flat_max_splits(a.njobs, a.nwg, _tiles(a)))),
                "head_dy": lambda a: F32 * a.N * 48 * a.H * a.W, "head_x16": lambda a: F32 * a.N * 16 * a.H * a.W,
                "head_partial": lambda a: _wgrad_partial(a, 48, 16, 1) * int(_lib().larva_wgrad_flat_head_splits(a.njobs, a.nwg, _tiles(a)))},
        "host": ("splits_out", "head_splits_out")},
    "larva_conv3x3_wgrad_partial": {
        "dev": {"dy": lambda a: F32 * a.N * a.cout * a.H * a.W, "x": lambda a: F32 * a.N * a.cin * a.H * a.W,
                "partial": lambda a: _wgrad_partial(a, a.cout, a.cin, max(1, min(a.splits, _tiles(a))))},
        "host": ("splits_used",)},
    "larva_wgrad_reduce": {"dev": dict(_REDUCE), "host": _REDUCE_HOST},
    "larva_wgrad_reduce_with_loss": {"dev": dict(_REDUCE, terms=lambda a: [F32 * c for c in a.count], loss_out=lambda a: F32),
                                     "host": _REDUCE_HOST + ("count", "scale")},
    "larva_loss_from_partials_to_host_seq": {
        "dev": {"terms": lambda a: [F32 * c for c in a.count], "out": lambda a: F32, "host_cell": lambda a: 8,
                "dev_seq": lambda a: 4}, "host": ("count", "scale")},
    "larva_l1_fwd": {"dev": {"a": lambda a: F32 * a.numel, "b": lambda a: F32 * a.numel, "partial": _l1_ws, "loss": lambda a: F32},
                     "host": ()},
    "larva_l1_bwd": {"dev": {"a": lambda a: F32 * a.numel, "b": lambda a: F32 * a.numel, "gout": lambda a: F32,
                             "ga": lambda a: F32 * a.numel}, "host": ()},
    "larva_l1_partial_grad": {"dev": {"a": lambda a: F32 * a.N * a.C * 16 * a.H * a.W, "b": lambda a: F32 * a.N * a.C * 16 * a.H * a.W,
                                      "partial": _l1_ws, "grad": lambda a: F32 * a.N * 16 * a.C * a.H * a.W},
                              "host": ("blocks_out",)},
    "larva_pixel_unshuffle4": {"dev": {"in": lambda a: F32 * a.N * a.C * 16 * a.H * a.W, "out": lambda a: F32 * a.N * 16 * a.C * a.H * a.W},
                               "host": ()},
    "larva_upsample4_fwd": {"dev": {"in": lambda a: F32 * a.N * a.C * a.H * a.W, "out": lambda a: F32 * a.N * a.C * 16 * a.H * a.W},
                            "host": ()},
    "larva_adamw_step_host": {"dev": dict(_ADAMW), "host": ()},
    "larva_gather_patches": {"dev": {"data": lambda a: TENSOR, "offsets": lambda a: TENSOR, "hw": lambda a: TENSOR,
                                     "draws": lambda a: 4 * 5 * a.B, "out": lambda a: F32 * a.B * 3 * a.P * a.P}, "host": ()},
    "larva_u8_hwc_to_f32_chw": {"dev": {"in": lambda a: a.N * a.H * a.W * 3, "out": lambda a: F32 * a.N * 3 * a.H * a.W}, "host": ()},
    "larva_f32_chw_to_u8_hwc": {"dev": {"in": lambda a: F32 * a.N * 3 * a.H * a.W, "out": lambda a: a.N * a.H * a.W * 3}, "host": ()},
    "larva_f16_pack_weights": {"dev": {"w": lambda a: F32 * a.cout * a.cin * 9, "wpk": lambda a: _f16_packed(a.cin // 48)}, "host": ()},
    "larva_f16_head": {"dev": {"x": lambda a: F32 * a.N * 3 * a.H * a.W, "w": lambda a: F32 * 48 * 27, "bias": lambda a: F32 * 48,
                               "out": _f16_act, "flag": lambda a: 4}, "host": ()},
    "larva_f16_conv3x3": {"dev": {"srcs": _f16_act, "wpk": lambda a: _f16_packed(a.nsrc), "bias": lambda a: F32 * 48, "res0": _f16_act,
                                  "res1": _f16_act, "out": _f16_act, "flag": lambda a: 4}, "host": ()},
    "larva_f16_conv3x3_shuffle_base_u8": {"dev": {"src": _f16_act, "wpk": lambda a: _f16_packed(1), "bias": lambda a: F32 * 48,
                                                  "base": _hr3, "out": lambda a: a.N * 16 * a.H * a.W * 3, "flag": lambda a: 4},
                                          "host": ()},
    "larva_resize_u8": {"dev": {"src": lambda a: a.N * a.H * a.W * 3, "dst": lambda a: a.N * a.h * a.w * 3,
                                "hbounds": lambda a: 4 * 2 * a.w, "hcoeffs": lambda a: 4 * a.kx * a.w,
                                "vbounds": lambda a: 4 * 2 * a.h, "vcoeffs": lambda a: 4 * a.ky * a.h}, "host": ()},
    "larva_i420_to_rgb_f32": {"dev": {"frames": _i420_bytes, "out": lambda a: F32 * a.N * 3 * a.H * a.W}, "host": ("coef_table",)},
    "larva_rgb_u8_to_i420": {"dev": {"img": lambda a: a.N * a.H * a.W * 3, "out": _i420_bytes}, "host": ("coef_table",)},
    "larva_rgba_u8_split_f32": {"dev": {"rgba": lambda a: a.N * a.H * a.W * 4, "alpha_slot": lambda a: 4 * a.N,
                                        "out": lambda a: F32 * (a.N + a.K) * 3 * a.H * a.W}, "host": ()},
    "larva_rgb_u8_merge_rgba": {"dev": {"rgb": lambda a: (a.N + a.K) * a.h * a.w * 3, "alpha_slot": lambda a: 4 * a.N,
                                        "out": lambda a: a.N * a.h * a.w * 4}, "host": ()},
}


class MissingFootprint(AssertionError):
    pass


class _Args:
    def __init__(self, values):
        self.__dict__.update(values)


def launch_record(name, params, args, footprints=None, tensors=None, **meta):
    """The access record of one library launch from its entry point's parameters and the ctypes arguments of the call:
    an int is a device pointer or a scalar, a ctypes array of pointers a host array of device operands, any other ctypes
    array a host array of scalars, anything else (byref) a host result.  The stream is the last argument."""
    fp = (FOOTPRINTS if footprints is None else footprints).get(name)
    if fp is None:
        raise MissingFootprint("no footprint declared for entry point %s: tests/stream_order.py FOOTPRINTS must state the "
                               "byte extent of each of its pointer operands" % name)
    if len(args) != len(params):
        raise AssertionError("%s: called with %d arguments, the header declares %d" % (name, len(args), len(params)))
    values = {}
    for p, v in zip(params, args):
        if isinstance(v, ctypes.Array):
            v = list(v)
        elif isinstance(v, (ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong, ctypes.c_uint)):
            v = v.value
        values[p.name] = v
    a = _Args(values)
    stream = args[-1] or 0
    reads, writes = [], []
    for p, v in zip(params[:-1], args[:-1]):
        if not p.pointer or v is None or p.name in fp["host"]:
            continue
        if isinstance(v, ctypes.Array) and v._type_ is ctypes.c_void_p:
            ptrs, many = list(v), True
        elif isinstance(v, int):
            ptrs, many = [v], False
        else:
            raise MissingFootprint("%s: pointer parameter `%s` was passed a host object (%s) but is not declared a host "
                                   "parameter of the entry point's footprint" % (name, p.name, type(v).__name__))
        if p.name not in fp["dev"]:
            raise MissingFootprint("%s: no extent declared for pointer parameter `%s`" % (name, p.name))
        extent = fp["dev"][p.name](a)
        for i, ptr in enumerate(ptrs):
            if ptr is None:
                continue
            n = extent[i] if isinstance(extent, (list, tuple)) else extent
            if n == TENSOR:
                n = (tensors or {}).get(ptr)
                if n is None:
                    raise MissingFootprint("%s: `%s` is a table sized by its tensor, and no tensor the recorder saw starts "
                                           "at %#x" % (name, p.name, ptr))
            (reads if p.const else writes).append([ptr, ptr + int(n), "%s[%d]" % (p.name, i) if many else p.name])
    return access(stream, name, reads, writes, **meta)


# ------------------------------------------------------------------------------------------------ the recorder
# torch operators that launch nothing: allocation without initialisation, metadata, aliases
_NO_LAUNCH = {"aten::empty.memory_format", "aten::empty_strided", "aten::empty_like", "aten::new_empty", "aten::new_empty_strided",
              "aten::detach", "aten::alias", "aten::lift_fresh", "aten::record_stream", "aten::is_pinned", "aten::set_.source_Storage",
              "aten::set_.source_Storage_storage_offset", "aten::set_.source_Tensor", "aten::resize_", "aten::is_same_size",
              "aten::_has_compatible_shallow_copy_type", "aten::sym_size.int", "aten::sym_stride.int", "aten::sym_numel",
              "aten::sym_storage_offset", "aten::dim", "aten::is_contiguous", "aten::stride.int", "aten::size.int", "aten::numel"}


def span(t):
    """[lo, hi) of the bytes a tensor's elements cover, or None for an empty one."""
    if t.numel() == 0:
        return None
    n = 1 + sum((int(s) - 1) * int(st) for s, st in zip(t.shape, t.stride()))
    return t.data_ptr(), t.data_ptr() + n * t.element_size()


def _site():
    """(file, function, line) of the first frame outside torch and this helper."""
    f = sys._getframe(2)
    here = os.path.abspath(__file__)
    while f is not None:
        name = f.f_code.co_filename
        if os.path.abspath(name) != here and os.sep + "torch" + os.sep not in name and "contextlib" not in name:
            return [os.path.basename(name), f.f_code.co_name, f.f_lineno]
        f = f.f_back
    return ["?", "?", 0]


class Recorder:
    """with Recorder(monkeypatch) as rec: ... ; rec.log is the log.  strict=False: an entry point without a footprint is
    noted in rec.missing instead of raising (a survey of what a scenario reaches; the tests run strict)."""

    def __init__(self, monkeypatch, strict=True):
        self.mp, self.strict = monkeypatch, strict
        self.log, self.missing = [], []
        self.tensors = {}            # data_ptr -> bytes of the cuda tensors torch made under the recorder
        self._keep = []              # events and graphs named in the log: their ids must not be reused
        self._tokens = {}
        self._tls = threading.local()
        self._lock = threading.Lock()
        self._backward = 0
        self._mode = None

    # -- plumbing
    def _add(self, rec):
        import torch.utils._python_dispatch as pd
        rec["thread"] = threading.get_ident()
        rec["bw"] = self._backward > 0
        rec["mode"] = pd._get_current_dispatch_mode() is not None or getattr(self._tls, "in_mode", False)
        with self._lock:
            self.log.append(rec)

    def _token(self, obj, prefix):
        key = id(obj)
        if key not in self._tokens:
            self._tokens[key] = "%s%d" % (prefix, len(self._tokens))
            self._keep.append(obj)
        return self._tokens[key]

    @staticmethod
    def _current():
        import torch
        return torch.cuda.current_stream().cuda_stream

    def _outer(self, owner, attr, after):
        """Patch owner.attr: call the original, then after(result, *args, **kwargs) -- only for the outermost patched
        call of a thread (Stream.wait_stream is Stream.wait_event of Stream.record_event: one edge, logged once)."""
        orig = getattr(owner, attr)
        tls = self._tls

        def wrapper(*args, **kwargs):
            outer = not getattr(tls, "busy", False)
            tls.busy = True
            try:
                result = orig(*args, **kwargs)
            finally:
                if outer:
                    tls.busy = False
            if outer:
                after(result, *args, **kwargs)
            return result
        wrapper.__name__ = attr
        self.mp.setattr(owner, attr, wrapper)

    # -- the four parts
    def __enter__(self):
        import torch
        from torch.utils._python_dispatch import TorchDispatchMode
        rec = self

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                out = func(*args, **(kwargs or {}))
                rec._tls.in_mode = True
                try:
                    rec._torch_op(func, args, kwargs or {}, out)
                finally:
                    rec._tls.in_mode = False
                return out

        self._patch_library()
        self._patch_ordering(torch)
        self._patch_pipeline()
        self._mode = Mode()
        self._mode.__enter__()
        return self

    def __exit__(self, *exc):
        self._mode.__exit__(*exc)
        return False

    # (1) library launches
    def _patch_library(self):
        from larvanet_amd import hip_lib
        lib = hip_lib.load()
        for name, params in parse_params(hip_lib.HEADER_PATH).items():
            if is_launch(params):
                self.mp.setattr(lib, name, self._launcher(name, getattr(lib, name), params))

    def _launcher(self, name, fn, params):
        def launch(*args):
            code = fn(*args)
            if code == 0:      # (anything else: nothing was launched, and the caller raises or takes another entry point)
                try:
                    self._add(launch_record(name, params, args, tensors=self.tensors, site=_site()))
                except MissingFootprint as e:
                    if self.strict:
                        raise
                    self.missing.append(str(e))
            return code
        launch.__name__ = name
        return launch

    # (2) torch's own device work
    def _torch_op(self, func, args, kwargs, out):
        import torch
        schema = func._schema
        name = schema.name + ("." + schema.overload_name if schema.overload_name else "")
        ins = []     # (tensor, label, is_write)
        for i, arg in enumerate(schema.arguments):
            v = args[i] if i < len(args) else kwargs.get(arg.name)
            w = arg.alias_info is not None and arg.alias_info.is_write
            for j, t in enumerate(v if isinstance(v, (list, tuple)) else [v]):
                if isinstance(t, torch.Tensor):
                    ins.append((t, arg.name if not isinstance(v, (list, tuple)) else "%s[%d]" % (arg.name, j), w))
        outs, views = [], 0
        flat = list(out) if isinstance(out, (list, tuple)) else [out]
        for i, t in enumerate(flat):
            if isinstance(t, torch.Tensor):
                info = schema.returns[min(i, len(schema.returns) - 1)].alias_info
                if info is not None and not info.is_write:
                    views += 1
                elif info is None:
                    outs.append((t, "out%d" % i if len(flat) > 1 else "out"))
        for t, _ in outs:
            if t.is_cuda and t.numel():
                s = span(t)
                self.tensors[s[0]] = max(self.tensors.get(s[0], 0), s[1] - s[0])
        if name in _NO_LAUNCH or (views and not outs and not any(w for _, _, w in ins)):
            return      # nothing is launched: an allocation, a question about metadata, a view
        tensors = [t for t, _, _ in ins] + [t for t, _ in outs]
        on_device = any(t.is_cuda for t in tensors)
        pinned = [t for t in tensors if t.device.type == "cpu" and t.numel() and t.is_pinned()]
        if not on_device and not pinned:
            return
        pinned_ids = {id(t) for t in pinned}

        def tracked(t):
            return t.numel() and (t.is_cuda or id(t) in pinned_ids)
        reads = [list(span(t)) + [label] for t, label, w in ins if not w and tracked(t)]
        writes = [list(span(t)) + [label] for t, label, w in ins if w and tracked(t)] + \
                 [list(span(t)) + [label] for t, label in outs if tracked(t)]
        if not on_device:    # the host alone, on pinned memory
            if reads or writes:
                self._add(host_access(reads, writes, name=name, site=_site()))
            return
        stream = self._current()
        self._add(access(stream, name, reads, writes, site=_site()))
        host_side = [t for t in tensors if t.device.type == "cpu"]
        result_on_host = not any(isinstance(t, torch.Tensor) for t in flat)    # .item(), equal(): a value comes back
        if host_side or result_on_host:
            non_blocking = bool(kwargs.get("non_blocking", False))
            for i, arg in enumerate(schema.arguments):
                if arg.name == "non_blocking" and i < len(args):
                    non_blocking = bool(args[i])
            asynchronous = non_blocking and not result_on_host and all(id(t) in pinned_ids for t in host_side)
            pageable_in = non_blocking and all(not t.is_cuda for t, _, w in ins if not w) and not any(id(t) in pinned_ids for t in host_side)
            if not asynchronous and not pageable_in:
                self._add(host_sync(stream=stream, origin=name, site=_site()))

    # (3) ordering calls
    def _patch_ordering(self, torch):
        S, E, G = torch.cuda.Stream, torch.cuda.Event, torch.cuda.CUDAGraph

        def stream_of(s):
            return self._current() if s is None else s.cuda_stream

        def on_wait_stream(_, self_, other):
            tok = "ws%d" % len(self.log)
            self._add(record(tok, other.cuda_stream, origin="wait_stream", site=_site()))
            self._add(wait(self_.cuda_stream, tok, origin="wait_stream", site=_site()))
        self._outer(S, "wait_stream", on_wait_stream)
        self._outer(S, "wait_event", lambda _, s, ev: self._add(wait(s.cuda_stream, self._token(ev, "e"), origin="wait_event", site=_site())))
        self._outer(S, "record_event", lambda ev, s, event=None: self._add(record(self._token(ev, "e"), s.cuda_stream, origin="record_event", site=_site())))
        self._outer(S, "synchronize", lambda _, s: self._add(host_sync(stream=s.cuda_stream, origin="Stream.synchronize", site=_site())))
        self._outer(E, "record", lambda _, ev, stream=None: self._add(record(self._token(ev, "e"), stream_of(stream), origin="Event.record", site=_site())))
        self._outer(E, "wait", lambda _, ev, stream=None: self._add(wait(stream_of(stream), self._token(ev, "e"), origin="Event.wait", site=_site())))
        self._outer(E, "synchronize", lambda _, ev: self._add(host_sync(event=self._token(ev, "e"), origin="Event.synchronize", site=_site())))
        self._outer(torch.cuda, "synchronize", lambda _, device=None: self._add(host_sync(origin="torch.cuda.synchronize", site=_site())))
        self._outer(G, "capture_begin", lambda _, g, *a, **k: self._add(capture_begin(self._token(g, "g"), self._current(), site=_site())))
        self._outer(G, "capture_end", lambda _, g: self._add(capture_end(self._token(g, "g"), site=_site())))
        self._outer(G, "replay", lambda _, g: self._add(replay(self._token(g, "g"), self._current(), site=_site())))

        def on_record_stream(_, t, stream):
            s = span(t)
            if s is not None:
                self._add(record_stream(s[0], s[1], stream.cuda_stream, site=_site()))
                log, lock = self.log, self._lock

                def died(lo=s[0], hi=s[1]):
                    with lock:
                        log.append(free(lo, hi))
                try:
                    weakref.finalize(t.untyped_storage(), died)
                except TypeError:
                    pass
        self._outer(torch.Tensor, "record_stream", on_record_stream)
        orig_backward = torch.Tensor.backward

        def backward(*a, **k):
            self._backward += 1
            try:
                return orig_backward(*a, **k)
            finally:
                self._backward -= 1
        self.mp.setattr(torch.Tensor, "backward", backward)

    # (4) the host side of the pipeline
    def _patch_pipeline(self):
        from larvanet_amd import pipeline
        orig_views = pipeline._Slot.views

        def views(slot, which, shape, host=True):
            got = orig_views(slot, which, shape, host)
            if host:
                s = span(got[0])
                if s is not None:
                    ops = [[s[0], s[1], "pin." + which]]
                    self._add(host_access(reads=ops if which == "out" else (), writes=() if which == "out" else ops,
                                          name="_Slot.views", site=_site()))
            return got
        self.mp.setattr(pipeline._Slot, "views", views)
        for cls in (pipeline._Stage, pipeline._EvaluateStage):
            self.mp.setattr(cls, "result", self._result(cls.result))

    def _result(self, orig):
        def result(stage, slot):
            if slot.pin_record is not None:
                s = span(slot.pin_record)
                self._add(host_access(reads=[[s[0], s[1], "pin.record"]], name="stage.result", site=_site()))
            self._add({"kind": "note", "text": "stage.result"})
            return orig(stage, slot)
        return result


def find(log, kind=None, origin=None, site=None):
    """Indices of the records of one kind / origin / site (file, function)."""
    out = []
    for i, r in enumerate(log):
        if kind is not None and r["kind"] != kind:
            continue
        if origin is not None and r.get("origin") != origin:
            continue
        if site is not None and tuple((r.get("site") or ["", ""])[:2]) != tuple(site):
            continue
        out.append(i)
    return out
