"""The road table of tests/test_gpu_avir_roads.py, tests/test_avir_road_table.py
and tools/avir_road_trace.py: one row per outcome of avir_road
(avir_amd/csrc/api.cpp) -- the attempts a call makes, in order -- the call
that walks it, and the stages and kernels its AVIRHIP_VERBOSE lines have to
name, in order (`tags`).

The tag lists were recorded once from a library built from the commit before
avir_road existed (profiles/avir_road/parent.txt), not read off the new code.

A row: `outcome` names a line of the comment table above avir_road; `module`
is the case module of tests/ its shape (sw, sh, nw, nh) is taken from, so that
the plan is known to be the family's; `soff` / `doff` / `spad`: bytes the
source / the destination start off their allocation's 64-byte grid, elements
added to the source row pitch; `rc`: the whole-frame call's return code when it
is not 0 -- such a row's destination stays untouched, and the automatic path
then serves the same pointers (`tags`: that call's)."""
import ctypes as C
import numpy as np
import avir_amd
from avir_amd import abi
from tests import helpers as H
from tests import refbind as rb
from tests import dnf16_cases as D16
from tests.gpass_route_cases import environment  # noqa: F401 (the test's)

T = dict(D16.T, f64=(abi.F64, np.float64))   # (f64: tests/lanc_road_cases.py)
GUARD = 0x5a
MAX_SRC_PIXELS = 600 * 402
P2, P3, P4, P5 = 2, 3, 4, abi.PATH_GPASS
K2S, K3S = (600, 400, 300, 200), (600, 402, 200, 134)   # dnsrgb8_cases K2, K3
D2, D3 = (600, 400, 300, 200), (600, 402, 200, 134)     # dnf16_cases K2, K3
X2 = (200, 48, 400, 96)                                 # window_cases
X2U = (322, 420, 644, 840)                              # ... with uint8 RGBA
GEN = (360, 500, 200, 278)                              # window_cases, path 1
PACK, OUT = "pack pass", "output stage"
MAXPIX = "AVIRHIP_DNSRGB_STORE_MAXPIX"

# the lines of the comment table above avir_road
OUTCOMES = ["k_dnfh sRGB", "k_dnfh 16-bit", "tiles", "k_up2 raw", "k_up2 store",
            "k_up2", "pass store", "pass", "generic"]

ROWS = []


def _row(name, outcome, module, geom, ch, tin, tout, path, tags, **kw):
    r = dict(name=name, outcome=outcome, module=module, geom=geom, ch=ch,
             tin=tin, tout=tout, path=path, tags=tags, variant=0, env={},
             soff=0, doff=0, spad=0, gamma=False, alpha=-1, errd=False, fp=1,
             bits=8 if tout == "u8" else 16, rc=0)
    assert set(kw) <= set(r), kw
    r.update(kw)
    ROWS.append(r)


# ---- k_dnfh with sRGB gamma (ResBitDepth 8, as tests/dnsrgb8_cases.py)
for _g, _n in ((K2S, "k2"), (K3S, "k3")):
    _s = dict(gamma=True, alpha=3, bits=8)
    _row("srgb_u8_u8_" + _n, "k_dnfh sRGB", "dnsrgb8_cases", _g, 4, "u8", "u8",
         0, ["k_dnfh"], **_s)
    _row("srgb_src_base1_" + _n, "k_dnfh sRGB", "dnsrgb8_cases", _g, 4, "u8",
         "u8", 0, [PACK, "k_dnfh"], soff=1, **_s)
    _row("srgb_store_alone_" + _n, "k_dnfh sRGB", "dnsrgb8_cases", _g, 3,
         "f32", "u8", P2, [PACK, "k_dnfh"], gamma=True, bits=8,
         env={MAXPIX: str(_g[0] * _g[1])})
    _row("srgb_store_alone_too_large_" + _n, "tiles", "dnsrgb8_cases", _g, 3,
         "f32", "u8", P2, [PACK, "k_dnf", OUT], gamma=True, bits=8,
         env={MAXPIX: str(_g[0] * _g[1] - 1)})
    _row("srgb_neither_side_" + _n, "tiles", "dnsrgb8_cases", _g, 4, "u8",
         "f32", 0, [PACK, "k_dnf"], soff=2, **_s)

# ---- k_dnfh with half / bfloat16 pixels; the tiles behind it
for _g, _n in ((D2, "k2"), (D3, "k3")):
    _row("dn16_f16_f16_" + _n, "k_dnfh 16-bit", "dnf16_cases", _g, 4, "f16",
         "f16", 0, ["k_dnfh"])
    _row("dn16_u8_f16_" + _n, "k_dnfh 16-bit", "dnf16_cases", _g, 4, "u8",
         "f16", 0, [PACK, "k_dnfh"])
    _row("dn16_f16_u8_" + _n, "k_dnfh 16-bit", "dnf16_cases", _g, 4, "f16",
         "u8", 0, ["k_dnfh"])
    _row("dn16_f16_u8_dst1_" + _n, "k_dnfh 16-bit", "dnf16_cases", _g, 4,
         "f16", "u8", 0, ["k_dnfh", OUT], doff=1)
    _row("dn16_odd_pitch_declined_" + _n, "tiles", "dnf16_cases", _g, 4, "f16",
         "f32", 0, [PACK, "k_dnf"], spad=1)
    _row("dn16_unfused_" + _n, "tiles", "dnf16_cases", _g, 4, "f16", "f16", P2,
         [PACK, "k_dnf", OUT], variant=abi.VARIANT_DN_UNFUSED_IO)
    _row("tiles_f32_u8_" + _n, "tiles", "dnf16_cases", _g, 4, "f32", "u8", P2,
         ["k_dnf"])
    _row("tiles_f32_u8_dst1_" + _n, "tiles", "dnf16_cases", _g, 4, "f32", "u8",
         P2, ["k_dnf", OUT], doff=1)
    _row("tiles_u8c3_path3_" + _n, "tiles", "dnf16_cases", _g, 3, "u8", "u8",
         P3, [OUT])

# ---- k_up2
_row("up2_u8c4", "k_up2 raw", "window_cases", X2U, 4, "u8", "u8", P4, ["k_up2"])
# (the short frame: the kernel refuses to store its uint8 pixels, and the call
# makes all three attempts of the path)
_row("up2_u8c4_short", "k_up2", "window_cases", X2, 4, "u8", "u8", P4,
     [PACK, "k_up2", OUT])
_row("up2_u16_odd_base", "k_up2 store", "window_cases", X2, 4, "u16", "u16",
     P4, [PACK, "k_up2"], soff=2)
_row("up2_u8c3_f32c3", "k_up2 store", "window_cases", X2, 3, "u8", "f32", P4,
     [PACK, "k_up2"])
_row("up2_f32", "k_up2", "window_cases", X2, 4, "f32", "f32", P4, ["k_up2"])
_row("up2_unfused", "k_up2", "window_cases", X2U, 4, "u8", "u8", P4,
     [PACK, "k_up2", OUT], variant=abi.VARIANT_UP2_UNFUSED_IO)
_row("up2_f16", "k_up2 raw", "window_cases", X2, 4, "f16", "f16", P4,
     ["k_up2"])
# (the automatic path's kernels print no line)
_row("up2_forced_dst4", "k_up2", "window_cases", X2, 4, "f32", "f32", P4,
     [], doff=4, rc=abi.EUNSUPPORTED)

# ---- the pass kernels
_row("gp_f16_both_fused", "pass store", "gp16_cases", (64, 48, 100, 77), 4,
     "f16", "f16", P5, ["k_gh", "k_gv"], variant=abi.VARIANT_UPG_TWO_PASS)
_row("gp_u8_f16_store", "pass store", "gp16_cases", (300, 200, 100, 67),
     4, "u8", "f16", P5, ["k_sacc2", "k_sacc2v"])
# (fewer than four elements up to the end of the last source row: `raw16` is
# false -- and the planner gives so small a source the generic chain's plan)
_row("gp_f16_tiny", "generic", "gp16_cases", (3, 40, 5, 61), 1, "f16", "f16",
     0, [PACK, OUT])
_row("gp_f32_f32", "pass", "gpass_route_cases", (300, 200, 100, 67), 4, "f32",
     "f32", P5, ["k_sacc", "k_sacc"])
_row("gp_u8c3_gather", "pass store", "gpass_route_cases", (64, 48, 100, 77), 3,
     "u8", "u8", P5, ["k_gh", "k_gv"])
_row("gp_u8c3_mixed", "pass store", "gpass_route_cases", (90, 300, 200, 120),
     3, "u8", "u8", P5, ["k_gh", "k_sacc2v"])

# ---- the generic chain
_row("generic_u8c3", "generic", "window_cases", GEN, 3, "u8", "u8", 1,
     [PACK, OUT])
_row("generic_errd", "generic", "window_cases", GEN, 3, "u8", "u8", 1,
     [PACK, OUT], errd=True)
_row("generic_fp4_gamma_f32", "generic", "window_cases", GEN, 4, "f32", "f32",
     1, [PACK, OUT], fp=4, gamma=True, alpha=3)

NAMES = [r["name"] for r in ROWS]


def row(name):
    return ROWS[NAMES.index(name)]


def module_shapes(module):
    """The (sw, sh, nw, nh) of a case module of tests/."""
    import importlib
    m = importlib.import_module("tests." + module)
    if module in ("dnsrgb8_cases", "dnf16_cases"):
        return set(m.SHAPES + m.EXTRA_SHAPES)
    if module == "window_cases":
        return set(tuple(c[1:5]) for c in m.CASES)
    if module == "gp16_cases":
        return set(v[0] for v in m.ROUTES.values()) | set(
            t[:4] for t in m.TINY + m.THIN)
    if module == "gpass_route_cases":
        return set(tuple(c[0][1:5]) for r in m.ROWS for c in r[1])
    raise KeyError(module)


# ---- inputs and expected bits -------------------------------------------------

_REF = {}


def source(r):
    sw, sh, nw, nh = r["geom"]
    if r["tin"] == "u16":
        return rb.lcg_u8((sh, sw, r["ch"]), seed=sw + sh).astype(np.uint16) * 257
    return D16.source((sh, sw, r["ch"]), r["tin"], seed=sw + sh)


def case(r):
    """(source, expected result): the reference once per distinct call, shared
    and read-only. Half / bfloat16: the reference on the exactly widened
    source, its float32 result narrowed (tests/dnf16_cases.py)."""
    sw, sh, nw, nh = r["geom"]
    rt = r["tout"] if r["tout"] in ("u8", "u16") else "f32"
    key = (r["geom"], r["ch"], r["tin"], rt, r["bits"], r["gamma"], r["alpha"],
           r["errd"], r["fp"])
    if key not in _REF:
        src = source(r)
        kw = dict(out_dtype=T[rt][1], resbits=r["bits"], gamma=r["gamma"],
                  alpha=r["alpha"], errd=r["errd"])
        if r["fp"] == 4:
            # (fpclass_float4: a class the reference alone has; without it
            # the row's bits stay unchecked, as H.need_ref lays down)
            ref = (rb.ref_avir(src, nw, nh, variant=1, **kw)
                   if H.need_ref("fpclass_float4") else np.zeros(0, T[rt][1]))
        else:
            ref = H.checker_avir(D16.as_f32(src, r["tin"]), nw, nh, **kw)
        src.setflags(write=False)
        ref.setflags(write=False)
        _REF[key] = (src, ref)
    src, ref = _REF[key]
    return src, D16.from_f32(ref, r["tout"])


def bands(r):
    """The calls of a row beside the whole frame: thirds and an odd band (the
    recursive ditherer runs whole frames only)."""
    if r["errd"] or r["rc"] != 0:
        return []
    b, odd = D16.bands(r["geom"][3])
    return b + ([odd] if odd is not None else [])


# ---- the calls ------------------------------------------------------------------

def plan(r, path=None):
    """-> (resizer: keeps the plan alive, plan)"""
    lib = abi.load()
    sw, sh, nw, nh = r["geom"]
    v = None
    if r["gamma"]:
        v = avir_amd.CImageResizerVars()
        v.UseSRGBGamma, v.AlphaIndex = 1, r["alpha"]
    obj = avir_amd.CImageResizer(r["bits"], aFpPack=r["fp"],
                                 aDitherer="errd" if r["errd"] else "def")
    p = obj.plan(sw, sh, nw, nh, r["ch"], 0.0, v, T[r["tin"]][0],
                 T[r["tout"]][0], sw * r["ch"] + r["spad"] if r["spad"] else 0)
    path = r["path"] if path is None else path
    abi.check(lib.avirhip_plan_set_path(p, path), "set_path %d" % path)
    abi.check(lib.avirhip_plan_set_variant(p, r["variant"]), "set_variant")
    return obj, p


def device_source(r, src):
    """The source `soff` bytes into a device allocation, rows `spad` elements
    longer than their pixels -> (tensor: keeps it alive, pointer)."""
    import torch
    sh, sw, ch = src.shape
    pitch = sw * ch + r["spad"]
    flat = np.zeros(sh * pitch, src.dtype)
    flat.reshape(sh, pitch)[:, :sw * ch] = src.reshape(sh, sw * ch)
    b = flat[:(sh - 1) * pitch + sw * ch].view(np.uint8)
    t = torch.zeros(64 + r["soff"] + b.size, dtype=torch.uint8, device="cuda:0")
    t[64 + r["soff"]:] = torch.from_numpy(b.copy()).to("cuda:0")
    return t, t.data_ptr() + 64 + r["soff"]


def out_shape(r):
    return (r["geom"][3], r["geom"][2], r["ch"])


def run(lib, p, r, sptr, calls):
    """Output rows `calls` into one image between guard bytes, 64 + `doff` in
    front of it and a row behind it -> (return codes, the image's bytes as a
    uint8 array, whether the guards are untouched)."""
    import torch
    front = 64 + r["doff"]
    nh, nw, ch = out_shape(r)
    rowb = nw * ch * np.dtype(T[r["tout"]][1]).itemsize
    nbytes = nh * rowb
    d = torch.full((front + nbytes + rowb,), GUARD, dtype=torch.uint8,
                   device="cuda:0")
    rcs = [lib.avirhip_resize_band(
        p, C.c_void_p(sptr), abi.MEM_DEVICE,
        C.c_void_p(d.data_ptr() + front + a * rowb), abi.MEM_DEVICE, a, b, None)
        for (a, b) in calls]
    torch.cuda.synchronize()
    g = d.cpu().numpy()
    clean = bool((g[:front] == GUARD).all() and
                 (g[front + nbytes:] == GUARD).all())
    return rcs, g[front:front + nbytes].copy(), clean
