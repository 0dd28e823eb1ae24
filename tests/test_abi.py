"""The C-ABI library loads on a machine without a GPU and exports exactly what include/larva_hip.h
declares (no compute calls here)."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


HEADERS = {"product": os.path.join(ROOT, "include", "larva_hip.h"), "diag": os.path.join(ROOT, "tools", "larva_diag.h")}
# every entry point a feature's tests name: the first kernels and each later feature's additions
MUST = ("larva_conv3x3_fwd", "larva_conv3x3_wgrad", "larva_pack_weights", "larva_bicubic4_fwd",
        "larva_l1_fwd", "larva_l1_bwd", "larva_pixel_unshuffle4", "larva_adamw_step",
        "larva_upsample_fwd", "larva_pixel_shuffle_base", "larva_pixel_unshuffle", "larva_l1_bwd_unshuffle",
        "larva_shuffle_l1_partial_grad",
        "larva_f16_packed_weight_halves", "larva_f16_pack_weights", "larva_f16_head", "larva_f16_conv3x3",
        "larva_f16_conv3x3_shuffle_base",
        "larva_u8_hwc_to_f32_chw", "larva_f32_chw_to_u8_hwc", "larva_f16_conv3x3_shuffle_base_u8",
        "larva_u8_metrics", "larva_u8_metrics_workspace_bytes",
        "larva_dihedral_inputs_u8", "larva_dihedral_inputs_f32", "larva_dihedral_mean",
        "larva_f16_conv3x3_jobs", "larva_f16_conv3x3_shuffle_base_jobs",
        "larva_i420_to_rgb_f32", "larva_rgb_u8_to_i420", "larva_resize_u8",
        "larva_rgba_u8_split_f32", "larva_rgb_u8_merge_rgba")
P, I, F, D, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong


def _declared(path=HEADERS["product"]):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(larva_[a-z0-9_]+)\s*\(", text)))


def _library():
    from larvanet_amd import hip_lib
    if not os.path.exists(hip_lib.LIB_PATH):
        from larvanet_amd.build import build_extension
        build_extension(verbose=False)
    return hip_lib.load()


def test_header_declares_the_expected_entry_points():
    names = _declared()
    for must in MUST:
        assert must in names


def test_entry_points_are_declared_bound_and_exported():
    from larvanet_amd import hip_lib
    declared, lib = _declared(), _library()
    for name in MUST:
        assert name in declared and name in hip_lib.SIGNATURES and hasattr(lib, name), name
    assert lib.larva_abi_version() == 5


@pytest.mark.parametrize("which", sorted(HEADERS))
def test_every_declared_name_has_a_signature(which):
    from larvanet_amd import hip_lib
    table = hip_lib.parse_header(HEADERS[which])
    assert sorted(table) == _declared(HEADERS[which]) and len(table) == {"product": 73, "diag": 10}[which]
    if which == "product":
        assert table == hip_lib.SIGNATURES
    else:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        try:
            import diag_lib
        finally:
            sys.path.pop(0)
        assert table == diag_lib.SIGNATURES


def test_types_are_read_from_the_header():
    from larvanet_amd.hip_lib import SIGNATURES
    assert SIGNATURES["larva_packed_weight_floats"][0] is LL and SIGNATURES["larva_wgrad_partial_floats"][0] is LL
    assert SIGNATURES["larva_error_string"] == (ctypes.c_char_p, [I])
    assert SIGNATURES["larva_abi_version"] == (I, [])
    assert SIGNATURES["larva_adamw_step_host_copy"] == (I, [P] * 4 + [I] + [D] * 5 + [F, LL] + [P] * 3)
    # const unsigned char* out, long long out_pitch, const unsigned char* truth, long long truth_pitch, six ints, ...
    assert SIGNATURES["larva_u8_metrics"] == (I, [P, LL, P, LL] + [I] * 6 + [P] * 3)
    # ..., int n, float divisor, float* out, float* host_cell, unsigned* dev_seq, void* stream
    assert SIGNATURES["larva_loss_from_partials_to_host_seq"] == (I, [P, P, P, I, F, P, P, P, P])
    assert SIGNATURES["larva_strip_tile_table"] == (I, [I, I, I, P, I])


@pytest.mark.parametrize("text, named", [("int larva_x(size_t n);", "size_t n"), ("status_t larva_x(int n);", "status_t"),
                                         ("int larva_x(void* p, n);", "larva_x"), ("int larva_x(int n) { return n; }", "larva_x"),
                                         ("int larva_x(int n);\nint larva_x(float n);", "larva_x"), ("struct s { int a; };", "int a")])
def test_parser_refuses_what_it_cannot_type(tmp_path, text, named):
    from larvanet_amd import hip_lib
    path = tmp_path / "bad.h"
    path.write_text("/* int larva_in_a_comment(size_t n); */\n#include <stddef.h>\nint larva_ok(const float* const* p, unsigned u); // fine\n" + text)
    with pytest.raises(RuntimeError, match=re.escape(named)):
        hip_lib.parse_header(str(path))
    path.write_text("void larva_ok(double d, long long n);\ntypedef struct t { int a; float* b[8]; } t;\n")
    assert hip_lib.parse_header(str(path)) == {"larva_ok": (None, [D, LL])}
    with pytest.raises(RuntimeError, match="nope.h is missing"):
        hip_lib.parse_header(str(tmp_path / "nope.h"))


def test_library_exports_every_declared_symbol():
    from larvanet_amd import hip_lib
    lib = _library()
    declared = _declared()
    assert sorted(hip_lib.SIGNATURES) == declared  # binding table and header agree
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.larva_abi_version() == 5
    # product entry points only: the measurement entry points (tools/larva_diag.h) exist in tools/_diag/*.so builds alone
    for name in ("larva_stamp_clock", "larva_delay_ticks", "larva_conv3x3_fwd_timed", "larva_conv3x3_fwd_strips_timed",
                 "larva_conv3x3_pair_chain_probe", "larva_conv3x3_chain_probe", "larva_maskbits_bytes"):
        assert name not in declared and not hasattr(lib, name), name
    # pure host-side size helpers need no device
    def stride(c):   # cout_stride() of csrc/larva_common.h: c itself where c % 32 is 16 (or 0: swizzled rows), else c + 16
        return c if c % 32 in (0, 16) else c + 16

    for cout, cin in ((48, 48), (64, 64), (32, 32), (48, 16), (48, 192), (48, 8)):
        # [cin/8] chunks x 9 taps x 8 channels x stride(cout) -- the layout include/larva_hip.h documents
        assert lib.larva_packed_weight_floats(cout, cin) == (cin // 8) * 9 * 8 * stride(cout), (cout, cin)
    assert lib.larva_wgrad_partial_floats(48, 48, 2) == 2 * (27 * 3 * 256 + 48)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from larvanet_amd import hip_lib
    monkeypatch.setattr(hip_lib, "_lib", None)
    monkeypatch.setattr(hip_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        hip_lib.load()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "larvanet_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(d, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(d, f)


def test_flat_wgrad_partition_covers_every_tile_once_within_the_advertised_image_counts():
    """The flat weight-gradient grid (larva_conv3x3_wgrad_partial_flat[_head]): workgroup w owns
    [G w / nwg, G (w + 1) / nwg) of the sequence of njobs x tiles tiles followed by the head's pseudo-tiles.  Replayed
    here in Python for seeded (njobs, nwg, tiles): every tile of every layer and of the head falls into exactly one
    share, and the workgroups touching a layer / the head never exceed what the two host-side size helpers
    (pure host code) tell the caller to allocate."""
    import random
    from larvanet_amd import hip_lib
    lib = hip_lib.load()
    rnd = random.Random(7)
    cases = [(40, 256, 256), (8, 256, 256), (1, 3, 96), (5, 7, 6), (64, 1024, 30), (3, 64, 2)]
    cases += [(rnd.randint(1, 64), rnd.randint(1, 600), rnd.randint(1, 400)) for _ in range(60)]
    for njobs, nwg, tiles in cases:
        for with_head in (False, True):
            hu = (tiles * 6 + 9) // 10 if with_head else 0   # (LARVA_HEAD_COST10 = 6: a head tile priced at 0.6 of a 48 -> 48 tile)
            T = njobs * tiles
            G = T + hu
            n = min(nwg, G)
            owners = [[] for _ in range(njobs)]
            covered = [0] * njobs
            head_owner, head_cov = [], 0
            for w in range(n):
                g0, g1 = G * w // n, G * (w + 1) // n
                g, g_end = g0, min(g1, T)
                while g < g_end:
                    jb = g // tiles
                    seg_end = min(g_end, (jb + 1) * tiles)
                    owners[jb].append(w)
                    covered[jb] += seg_end - g
                    g = seg_end
                if hu and g1 > T:
                    p0, p1 = max(g0, T) - T, g1 - T
                    head_owner.append(w)
                    head_cov += p1 * tiles // hu - p0 * tiles // hu
            assert covered == [tiles] * njobs, (njobs, nwg, tiles, with_head)
            cap = lib.larva_wgrad_flat_max_splits(njobs, nwg, tiles)
            assert all(o == list(range(o[0], o[0] + len(o))) and len(o) <= cap for o in owners), (njobs, nwg, tiles)
            if with_head:
                assert head_cov == tiles and head_owner == list(range(head_owner[0], n)), (njobs, nwg, tiles)
                assert len(head_owner) == lib.larva_wgrad_flat_head_splits(njobs, nwg, tiles), (njobs, nwg, tiles)

