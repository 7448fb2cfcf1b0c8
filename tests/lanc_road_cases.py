"""The road table of tests/test_gpu_lanc_roads.py, tests/test_lanc_road_table.py
and tools/avir_road_trace.py --cases lanc: one row per attempt of lanc_road
(avir_amd/csrc/api.cpp) -- the attempts a CLancIR call makes, in order -- the
call that walks it, and the stages and kernels its AVIRHIP_VERBOSE lines have
to name, in order (`tags`).

The tag lists were recorded once from a library built from the commit before
lanc_road existed (profiles/lanc_road/parent.txt), not read off the new code.

A row is tests/avir_road_cases.py's: `outcome` names a line of the comment
table above lanc_road -- the attempt that takes the call; `module` is the
module of tests/ its shape (sw, sh, nw, nh) is taken from; `soff` / `doff` /
`spad`, `rc` as there. Expected bits: the reference's CLancIR
(tests/helpers.py, checker_lancir), 16-bit expectations as
tests/lancgp16_cases.py defines them."""
import collections
import numpy as np
from avir_amd import abi
from tests import helpers as H
from tests import refbind as rb
from tests import align_cases as A
from tests import dnf16_cases as D16
from tests import lancgp16_cases as L16
from tests import avir_road_cases as AR
from tests.avir_road_cases import (environment, device_source, run,  # noqa: F401
                                   out_shape, bands, GUARD, PACK, OUT)

T = AR.T
MAX_SRC_PIXELS = 600 * 402
P4, P5 = 4, abi.PATH_GPASS
UP, DN18, MIXED, TALL, NARROW = L16.UP, L16.DN18, L16.MIXED, L16.TALL, L16.NARROW
X2H = (97, 61, 194, 122)        # test_gpu_lanc2h's (97, 61), exact 2x
LX2, LOWN, DN27 = A.LX2, A.LOWN, A.DN27
# The automatic path is 4 only from 1 500 000 source pixels on
# (finalize_lancir_plan): the smallest frame at which that decision can go
# wrong, and the one row above MAX_SRC_PIXELS.
AUTO4 = (1500, 1000, 3000, 2000)
LARGE = ["auto4_u8c4"]

# the lines of the comment table above lanc_road
OUTCOMES = ["k_lanc2h", "k_lanc2 raw", "k_lanc2", "pass raw", "pass", "generic"]

ROWS = []


def _row(name, outcome, module, geom, ch, tin, tout, path, tags, **kw):
    r = dict(name=name, outcome=outcome, module=module, geom=geom, ch=ch,
             tin=tin, tout=tout, path=path, tags=tags, variant=0, env={},
             soff=0, doff=0, spad=0, errd=False, rc=0)
    assert set(kw) <= set(r), kw
    r.update(kw)
    ROWS.append(r)


# ---- k_lanc2h: exact 2x RGBA, half / bfloat16 pixels on a side
for _t in ("f16", "bf16"):
    for _p in (0, P4):
        _row("lanc2h_%s_path%d" % (_t, _p), "k_lanc2h", "test_gpu_lanc2h", X2H,
             4, _t, _t, _p, ["k_lanc2h"])
_row("lanc2h_u8_f16", "k_lanc2h", "test_gpu_lanc2h", X2H, 4, "u8", "f16", 0,
     [PACK, "k_lanc2h"])
_row("lanc2h_f16_f32_unity", "k_lanc2h", "test_gpu_lanc2h", X2H, 4, "f16",
     "f32", 0, ["k_lanc2h"])
_row("lanc2h_f16_odd_pitch", "k_lanc2h", "test_gpu_lanc2h", X2H, 4, "f16",
     "f16", 0, [PACK, "k_lanc2h"], spad=1)
# (an exact-2x plan forced to path 5 is offered neither 16-bit type: `io16`)
_row("x2_f16_forced_5", "pass", "align_cases", LX2, 4, "f16", "f16", P5,
     [PACK, "k_lf", OUT])

# ---- k_lanc2
_row("lanc2_f16_u8", "k_lanc2", "align_cases", LX2, 4, "f16", "u8", P4,
     [PACK, "k_lanc2"])
_row("lanc2_u8c4", "k_lanc2 raw", "align_cases", LX2, 4, "u8", "u8", P4,
     ["k_lanc2"])
_row("lanc2_u8c3", "k_lanc2 raw", "align_cases", LX2, 3, "u8", "u8", P4,
     ["k_lanc2"])
_row("lanc2_u16c4", "k_lanc2 raw", "align_cases", LX2, 4, "u16", "u16", P4,
     ["k_lanc2"])
_row("lanc2_u8c4_f32", "k_lanc2 raw", "align_cases", LX2, 4, "u8", "f32", P4,
     ["k_lanc2"])
# (`dst2` is false: the float copy, and the fused store behind it)
_row("lanc2_u8c4_dst1", "k_lanc2", "align_cases", LX2, 4, "u8", "u8", P4,
     [PACK, "k_lanc2"], doff=1)
_row("lanc2_u16c4_src2", "k_lanc2", "align_cases", LX2, 4, "u16", "u16", P4,
     [PACK, "k_lanc2"], soff=2)
_row("lanc2_unfused", "k_lanc2", "align_cases", LX2, 4, "u8", "u8", P4,
     [PACK, "k_lanc2", OUT], variant=abi.VARIANT_UP2_UNFUSED_IO)
_row("lanc2_f64", "k_lanc2", "align_cases", LX2, 4, "f64", "f64", P4,
     [PACK, "k_lanc2", OUT])
_row("lanc2_f32", "k_lanc2", "align_cases", LX2, 4, "f32", "f32", P4,
     ["k_lanc2"])
# (the automatic path of so small a frame is the pass kernels', which refuse
# the same pointer: the generic kernels print no line)
_row("lanc2_f32_forced_dst4", "k_lanc2", "align_cases", LX2, 4, "f32", "f32",
     P4, [], doff=4, rc=abi.EUNSUPPORTED)
_row("auto4_u8c4", "k_lanc2 raw", "finalize_lancir_plan", AUTO4, 4, "u8", "u8",
     0, ["k_lanc2"])

# ---- the pass kernels
# (rows of 97 RGB uint8 pixels are 291 bytes: no dword pitch, and the loaders
# that move rows as bytes ask one -- lfuse.hip:462, gpassv.hip:50: the pack
# pass comes first; LOWN's rows of 384 bytes are read where they lie)
_row("pass_u8c3_up", "pass", "lancgp16_cases", UP, 3, "u8", "u8", P5,
     [PACK, "k_lf"])
_row("pass_u8c3_up_two_pass", "pass", "lancgp16_cases", UP, 3, "u8", "u8",
     P5, [PACK, "k_gv", "k_gh"], variant=abi.VARIANT_UPG_TWO_PASS)
_row("pass_u8c3_lown", "pass raw", "align_cases", LOWN, 3, "u8", "u8", P5,
     ["k_lf"])
_row("pass_u8c3_lown_two_pass", "pass raw", "align_cases", LOWN, 3, "u8", "u8",
     P5, ["k_gv", "k_gh"], variant=abi.VARIANT_UPG_TWO_PASS)
_row("pass_u16c4_lown", "pass raw", "align_cases", LOWN, 4, "u16", "u16", P5,
     ["k_lf"])
_row("pass_u8c4_x2_auto", "pass raw", "align_cases", LX2, 4, "u8", "u8", 0,
     ["k_lf"])
_row("pass_u8c4_dn27_auto", "pass raw", "align_cases", DN27, 4, "u8", "u8", 0,
     ["k_gv", "k_gh"])
_row("pass_f32c3_lown", "pass raw", "align_cases", LOWN, 3, "f32", "f32", P5,
     ["k_lf"])
_row("pass_f16_dn18", "pass raw", "lancgp16_cases", DN18, 4, "f16", "f16", 0,
     ["k_gv", "k_gh"])
_row("pass_bf16_up", "pass raw", "lancgp16_cases", UP, 4, "bf16", "bf16", P5,
     ["k_lf"])
_row("pass_f16_bf16_mixed", "pass raw", "lancgp16_cases", MIXED, 4, "f16",
     "bf16", 0, ["k_gv", "k_gh"])
_row("pass_u8_f16_up", "pass raw", "lancgp16_cases", UP, 4, "u8", "f16", P5,
     ["k_lf"])
_row("pass_f16_u8_up", "pass raw", "lancgp16_cases", UP, 4, "f16", "u8", P5,
     ["k_lf"])
_row("pass_f16_tall", "pass", "lancgp16_cases", TALL, 4, "f16", "f16", P5,
     [PACK, "k_gv", "k_gh"])
_row("pass_f16_narrow", "pass", "lancgp16_cases", NARROW, 4, "f16", "f16", P5,
     [PACK, "k_lf"])
_row("pass_f16_odd_base", "pass raw", "lancgp16_cases", UP, 4, "f16", "f16",
     P5, ["k_lf", OUT], doff=1)
_row("pass_f16_no_io16", "pass", "lancgp16_cases", UP, 4, "f16", "f16", P5,
     [PACK, "k_lf", OUT], env={"AVIRHIP_GP_NO_IO16": "1"})
_row("pass_f32_up", "pass", "lancgp16_cases", UP, 4, "f32", "f32", P5,
     ["k_lf"])
_row("pass_f32_dn27_auto", "pass", "align_cases", DN27, 4, "f32", "f32", 0,
     ["k_gv", "k_gh"])
_row("pass_f32_forced_src4", "pass", "lancgp16_cases", UP, 4, "f32", "f32",
     P5, [], soff=4, rc=abi.EUNSUPPORTED)

# ---- the generic kernels (they print no line)
_row("generic_owner_path1", "generic", "align_cases", LOWN, 3, "u8", "u8", 1,
     [])
_row("generic_f32_path1", "generic", "align_cases", DN27, 4, "f32", "f32", 1,
     [])

NAMES = [r["name"] for r in ROWS]


def row(name):
    return ROWS[NAMES.index(name)]


def module_shapes(module):
    """The (sw, sh, nw, nh) a row may take from a module of tests/."""
    if module == "lancgp16_cases":
        return {UP, DN18, MIXED, TALL, NARROW}
    if module == "test_gpu_lanc2h":
        from tests import test_gpu_lanc2h as M
        assert (97, 61) in M.SHAPES
        return {X2H}
    if module == "align_cases":
        return {LX2, LOWN, DN27}
    if module == "finalize_lancir_plan":
        return {AUTO4}
    raise KeyError(module)


# ---- inputs and expected bits -------------------------------------------------

_REF = {}


def _case64(r):
    sw, sh, nw, nh = r["geom"]
    key = (r["geom"], r["ch"])
    if key not in _REF:
        src = rb.lcg_f32((sh, sw, r["ch"]), seed=sw + sh).astype(np.float64)
        ref = H.checker_lancir(src, nw, nh, out_dtype=np.float64)
        src.setflags(write=False)
        ref.setflags(write=False)
        _REF[key] = (src, ref)
    return _REF[key]


def case(r):
    """(source, expected result): tests/lancgp16_cases.py's, the reference once
    per distinct call, shared and read-only."""
    if r["tin"] == "f64":
        return _case64(r)
    return L16.case(r["geom"], r["tin"], r["tout"], r["ch"])


def source(r):
    return case(r)[0] if r["tin"] == "f64" else L16.source(
        (r["geom"][1], r["geom"][0], r["ch"]), r["tin"],
        seed=r["geom"][0] + r["geom"][1] + r["ch"])


def same(got, want, tout, what):
    """Word for word; NaN == NaN whatever the payload."""
    if tout != "f64":
        return D16.same(got.view(want.dtype), want, tout, what)
    got = got.view(np.float64).reshape(want.shape)
    bad = (got.view(np.uint64) != want.view(np.uint64)) & ~(
        np.isnan(got) & np.isnan(want))
    n = int(bad.sum())
    print("%s: %d of %d elements differ" % (what, n, want.size))
    assert n == 0, "%s: %d of %d elements differ" % (what, n, want.size)


# ---- the calls ------------------------------------------------------------------

_Level = collections.namedtuple("_Level", "g spad dpad")


def plan(r, path=None):
    """-> (front end: keeps the plan alive, plan): tests/align_cases.py's
    CLancIR front end, the source rows `spad` elements longer."""
    lib = abi.load()
    sw, sh, nw, nh = r["geom"]
    q = dict(fe="lancir", sw=sw, sh=sh, nw=nw, nh=nh, ch=r["ch"], geom2=None,
             ex={}, bits=0)
    obj, arg = A.front_end(q, _Level(0, r["spad"], 0))
    p = obj.plan(sw, sh, nw, nh, r["ch"], arg, T[r["tin"]][0], T[r["tout"]][0])
    path = r["path"] if path is None else path
    abi.check(lib.avirhip_plan_set_path(p, path), "set_path %d" % path)
    abi.check(lib.avirhip_plan_set_variant(p, r["variant"]), "set_variant")
    return obj, p
