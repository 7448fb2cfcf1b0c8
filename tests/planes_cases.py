"""The case table of tests/test_gpu_planes.py (CLancIR over single-channel
planes: avirhip_lancir_resize_planes, k_lancp of avir_amd/csrc/lancp.hip) and
what its host-only check, tests/test_planes_table.py, needs to read it.

A row is one call: `planes` planes of one geometry (sw, sh, nw, nh), element
types `tin` / `tout` (names of tests/dnf16_cases.py's T, plus "f64"), laid out
with `gap` elements of padding behind every plane on both sides (0: the call
passes plane strides of 0, tightly packed), rows `spad` / `npad` elements
longer than their pixels (SrcSSize / NewSSize), the source base `soff` bytes
off its natural alignment, `far`: a plane stride in BYTES on both sides
instead of `gap`. `par` are (la, kx, ky, ox, oy). `road` is the line the call
has to print under AVIRHIP_VERBOSE: "k_lancp", or "fallback" for the classes
the kernel declines -- no other row may show the fallback line.

Expected bits: the reference's CLancIR (tests/helpers.py, checker_lancir) on
each plane as an (H, W, 1) image; half / bfloat16 as tests/lancgp16_cases.py
defines them (the float32 call on the exactly widened source, narrowed to
nearest even). Device buffers lie between guard bytes (0x5a), and every byte
that is no pixel of a result row is a guard byte: what comes back is compared
byte for byte with an image of the expected buffer.

The seam rows follow the kernel's tile (LP_TW x LP_TR output pixels), read out
of lancp.hip."""
import ctypes as C
import os
import re
import numpy as np
import avir_amd
from avir_amd import abi
from tests import helpers as H
from tests import dnf16_cases as D16
from tests import lancgp16_cases as L16

T = dict(D16.T, f64=(abi.F64, np.float64))
GUARD = 0x5a
FRONT = 64
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "avir_amd", "csrc")
DEF = (3.0, 0.0, 0.0, 0.0, 0.0)      # la, kx, ky, ox, oy
MAXPLANES = 6


def parse_constants(csrc=CSRC):
    """LP_TW, LP_TR, LP_LDS as lancp.hip defines them."""
    text = open(os.path.join(csrc, "lancp.hip")).read()
    out = {}
    for name in ("LP_TW", "LP_TR", "LP_LDS"):
        m = re.search(r"^#define %s (\d+)\b" % name, text, re.M)
        assert m, "lancp.hip: no #define %s" % name
        out[name] = int(m.group(1))
    return out


K = parse_constants()
TW, TR = K["LP_TW"], K["LP_TR"]

# ---- geometries ---------------------------------------------------------------
UP = (37, 23, 61, 40)        # kl 6, 6: kl % 4 == 2
DN2 = (48, 36, 24, 18)       # k = 2: kl 12, 12, no tail
DN15 = (60, 45, 40, 30)      # k = 1.5: kl 10, 10
DN3 = (70, 50, 23, 17)       # kl 20, 18
MIX_DU = (21, 33, 13, 70)    # down on x, up on y
MIX_UD = (66, 40, 99, 27)    # the reverse
CROP = (64, 48, 50, 40)      # with kx, ky, ox, oy
TINY = (9, 7, 6, 5)          # smaller than any tile
ROUND5 = (40, 30, 62, 45)
K16 = (400, 300, 25, 19)     # k = 16: 96 taps
LONGK = (1100, 60, 64, 20)   # k = 17.2 along x: 104 taps under a whole tile
CROP_PAR = (3.0, 0.8, 0.9, 4.25, 2.5)
LA2 = (2.0, 0.0, 0.0, 0.0, 0.0)

# kernel lengths per axis (x, y) the tap classes must have
TAPS = {"tap_up": (6, 6), "tap_dn2": (12, 12), "tap_dn15": (10, 10),
        "tap_dn3": (20, 18), "tap_up_la2": (4, 4)}

SEAM_SRC = (50, 20)
SEAMS = [("seam_m1", TW - 1, TR - 1), ("seam_0", TW, TR),
         ("seam_p1", TW + 1, TR + 1), ("seam_many", 2 * TW + 5, 2 * TR + 3)]

PAIRS = [("u8", "u8"), ("u8", "f32"), ("u8", "u16"), ("u16", "u16"),
         ("u16", "u8"), ("f32", "f32"), ("f32", "u8"), ("f16", "f16"),
         ("bf16", "bf16"), ("f16", "u8"), ("f32", "bf16")]
TYPE_GEOMS = [("up", UP), ("dn3", DN3)]

# constant float32 planes of value float32( n + 0.5 ) / float32( 255 ) with
# uint8 results: (geometry, n, elements that differ under the wrong rounding
# rule in the whole groups of four, in the tail)
ROUNDING = [(UP, 40, 956, 40), (MIX_DU, 88, 690, 70), (DN3, 66, 323, 51),
            (TINY, 24, 20, 10), (ROUND5, 0, 2490, 90)]

ROWS = []


def _row(name, geom, tin="u8", tout="u8", planes=3, road="k_lancp", **kw):
    r = dict(name=name, geom=geom, tin=tin, tout=tout, planes=planes,
             road=road, gap=0, spad=0, npad=0, soff=0, far=0, par=DEF,
             const=None)
    assert set(kw) <= set(r), kw
    r.update(kw)
    ROWS.append(r)


# ---- tap classes
_row("tap_up", UP)
_row("tap_dn2", DN2)
_row("tap_dn15", DN15)
_row("tap_dn3", DN3)
_row("tap_up_la2", UP, par=LA2)
_row("tap_down_x_up_y", MIX_DU)
_row("tap_up_x_down_y", MIX_UD)
_row("tap_crop", CROP, par=CROP_PAR)
_row("tap_tiny", TINY)
TAP_ROWS = [r["name"] for r in ROWS]

# ---- tile seams
for _n, _w, _h in SEAMS:
    _row(_n, SEAM_SRC + (_w, _h), planes=2)

# ---- element types
for _g, _geom in TYPE_GEOMS:
    for _a, _b in PAIRS:
        _row("type_%s_%s_%s" % (_g, _a, _b), _geom, _a, _b, planes=2)

# ---- plane counts and strides
for _n in (1, 3, 5):
    _row("planes%d_packed" % _n, UP, planes=_n)
    _row("planes%d_gap7" % _n, UP, planes=_n, gap=7)
    for _p in (1, 2, 3):
        _row("planes%d_pitch%d" % (_n, _p), UP, planes=_n, spad=_p, npad=_p)

# ---- the rounding rule
for _geom, _nv, _a, _b in ROUNDING:
    _row("round_%dx%d_n%d" % (_geom[2], _geom[3], _nv), _geom, "f32", "u8",
         planes=2, const=_nv)

# ---- far planes: a plane offset beyond 32 bits' reach
_row("far_planes", UP, planes=2, far=2 ** 31 + 64)

# ---- the classes lancp_run may decline
_row("k16", K16, planes=2, road=None)   # (decided by lds_of below)
_row("long_kernel", LONGK, planes=2, road="fallback")
_row("f64", UP, "f64", "f64", planes=2, road="fallback")
_row("f16_odd_base", UP, "f16", "f16", planes=2, soff=1, road="fallback")

NAMES = [r["name"] for r in ROWS]
FALLBACK_MAY = ["k16", "long_kernel", "f64", "f16_odd_base"]
CROSS = ["tap_up", "tap_dn3", "type_up_f16_f16"]
STREAM_ROW, NUMPY_ROW, TENSOR6 = "tap_dn15", "tap_up_x_down_y", UP


def row(name):
    return ROWS[NAMES.index(name)]


# ---- parameters, plans (host only) -------------------------------------------

def params(r):
    la, kx, ky, ox, oy = r["par"]
    sw, sh, nw, nh = r["geom"]
    p = avir_amd.CLancIRParams(sw + r["spad"] if r["spad"] else 0,
                               nw + r["npad"] if r["npad"] else 0, kx, ky, ox,
                               oy)
    p.la = la
    return p


def axes(r):
    """((kl, start list) of x, of y) from the host planner."""
    lib = abi.load()
    h = C.c_void_p()
    abi.check(lib.avirhip_lancir_create(C.byref(h)), "lancir_create")
    d = C.POINTER(abi.LancirDesc)()
    sw, sh, nw, nh = r["geom"]
    p = params(r)
    try:
        abi.check(lib.avirhip_lancir_build_desc(
            h, sw, sh, nw, nh, 1, C.byref(p), T[r["tin"]][0], T[r["tout"]][0],
            C.byref(d)), "build_desc")
        out = []
        for a in (d.contents.h, d.contents.v):
            out.append((a.kernel_len,
                        [a.pos[j].so - a.padl for j in range(a.dst_len)]))
        lib.avirhip_lancir_desc_free(d)
    finally:
        lib.avirhip_lancir_destroy(h)
    return out


def lds_of(r):
    """The LDS bytes lancp_run's rule gives the row's tile (restated: it
    chooses which line the k = 16 row expects, nothing else)."""
    (kl, st), _ = axes(r)
    sw, nw = r["geom"][0], r["geom"][2]
    span = 1
    for j0 in range(0, nw, TW):
        j1 = min(j0 + TW, nw)
        c0 = min(max(st[j0], 0), sw - 1)
        c1 = min(max(st[j1 - 1] + kl - 1, 0), sw - 1)
        span = max(span, c1 - c0 + 1)
    return TR * (span + (span >> 5) + 1) * 4


def road(r):
    if r["road"] is not None:
        return r["road"]
    return "k_lancp" if lds_of(r) <= K["LP_LDS"] else "fallback"


# ---- inputs and expected bits ---------------------------------------------------

_SRC, _REF = {}, {}


def _rt(tout):
    return tout if tout in ("u8", "u16", "f64") else "f32"


def sources(r):
    """(MAXPLANES, sh, sw) source planes of the row's type, shared."""
    sw, sh = r["geom"][:2]
    key = (sw, sh, r["tin"], r["const"])
    if key not in _SRC:
        if r["const"] is not None:
            v = np.float32(r["const"] + 0.5) / np.float32(255)
            a = np.full((MAXPLANES, sh, sw), v, np.float32)
        elif r["tin"] == "f64":
            a = L16.source((MAXPLANES, sh, sw), "f32",
                           seed=sw + sh).astype(np.float64)
        else:
            a = L16.source((MAXPLANES, sh, sw), r["tin"], seed=sw + sh + 1)
        a.setflags(write=False)
        _SRC[key] = a
    return _SRC[key]


def reference(r, i, rt=None):
    """The reference's result plane `i` in elements of class `rt` (float32,
    uint8, uint16, float64), once per distinct call."""
    rt = rt or _rt(r["tout"])
    key = (r["geom"], r["tin"], rt, r["par"], r["const"], i)
    if key not in _REF:
        la, kx, ky, ox, oy = r["par"]
        sw, sh, nw, nh = r["geom"]
        src = sources(r)[i].reshape(sh, sw, 1)
        ref = H.checker_lancir(L16.ref_input(src, r["tin"]), nw, nh,
                               out_dtype=T[rt][1], kx=kx, ky=ky, ox=ox, oy=oy,
                               la=la)
        ref = np.ascontiguousarray(ref).reshape(nh, nw)
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def expected(r, i):
    return D16.from_f32(reference(r, i), r["tout"])


def wrong_rule_counts(r):
    """How many elements of plane 0 the wrong rounding rule gets wrong: the
    reference's float32 result with + 0.5 truncation in the whole groups of
    four, nearest even in the tail, against its uint8 result -> (groups,
    tail)."""
    f = reference(r, 0, "f32")
    u = reference(r, 0, "u8")
    nw = r["geom"][2]
    l4 = nw & ~3
    v = np.clip(f * np.float32(255), np.float32(0), np.float32(255))
    trunc = (v + np.float32(0.5)).astype(np.int32)
    even = np.rint(v).astype(np.int32)
    return (int((trunc[:, :l4] != u[:, :l4]).sum()),
            int((even[:, l4:] != u[:, l4:]).sum()))


# ---- layout ---------------------------------------------------------------------

def side(r, which):
    """(w, h, pitch, stride passed to the call, stride in force, element
    size) of a side, strides and pitch in elements."""
    sw, sh, nw, nh = r["geom"]
    w, h, pad, t = ((sw, sh, r["spad"], r["tin"]) if which == "src" else
                    (nw, nh, r["npad"], r["tout"]))
    es = np.dtype(T[t][1]).itemsize
    pitch = w + pad
    need = (h - 1) * pitch + w
    if r["far"]:
        assert r["far"] % es == 0
        return w, h, pitch, r["far"] // es, r["far"] // es, es
    if r["gap"]:
        return w, h, pitch, need + r["gap"], need + r["gap"], es
    return w, h, pitch, 0, h * pitch, es


def _place(buf, off, plane, pitch):
    """Rows of `plane` (h, w) into the byte buffer at `off`, `pitch` elements
    apart."""
    h, w = plane.shape
    b = np.ascontiguousarray(plane).view(np.uint8).reshape(h, -1)
    es = plane.dtype.itemsize
    for y in range(h):
        o = off + y * pitch * es
        buf[o:o + w * es] = b[y]


def regions(r, which, planes):
    """The device image of a side as [(byte offset behind the base, bytes)]:
    guard bytes with the rows of `planes` in them, FRONT guard bytes in front
    of the first plane and behind the last. One region, or one per plane for
    far planes. `planes` None: guards only."""
    w, h, pitch, _, stride, es = side(r, which)
    n = r["planes"]
    need = ((h - 1) * pitch + w) * es
    if r["far"]:
        out = []
        for i in range(n):
            b = np.full(FRONT + need + FRONT, GUARD, np.uint8)
            if planes is not None:
                _place(b, FRONT, planes[i], pitch)
            out.append((i * stride * es - FRONT, b))
        return out
    b = np.full(FRONT + (n - 1) * stride * es + need + FRONT, GUARD, np.uint8)
    if planes is not None:
        for i in range(n):
            _place(b, FRONT + i * stride * es, planes[i], pitch)
    return [(-FRONT, b)]


def device_side(r, which, planes):
    """-> (tensor: keeps it alive, base pointer of plane 0)"""
    import torch
    regs = regions(r, which, planes)
    lo = min(o for o, b in regs)
    hi = max(o + b.size for o, b in regs)
    off = (r["soff"] if which == "src" else 0) + 64
    t = torch.empty(off + hi - lo, dtype=torch.uint8, device="cuda:0")
    for o, b in regs:
        t[off + o - lo:off + o - lo + b.size] = torch.from_numpy(b).to("cuda:0")
    return t, t.data_ptr() + off - lo


def read_back(r, t):
    """The result side's regions as they are on the device."""
    regs = regions(r, "dst", None)
    lo = min(o for o, b in regs)
    return [t[64 + o - lo:64 + o - lo + b.size].cpu().numpy() for o, b in regs]


def compare(r, got, what):
    """Byte for byte against the expected image: pixels and guards."""
    want = regions(r, "dst", [expected(r, i) for i in range(r["planes"])])
    mask = regions(r, "dst", [np.zeros_like(expected(r, i))
                              for i in range(r["planes"])])
    bad_px = bad_guard = 0
    for g, (o, w_), (o2, m) in zip(got, want, mask):
        px = (m != GUARD) | (w_ != GUARD)   # (a pixel byte may equal GUARD)
        d = g != w_
        bad_px += int((d & px).sum())
        bad_guard += int((d & ~px).sum())
    print("%s: %d pixel bytes differ, %d guard bytes written" % (
        what, bad_px, bad_guard))
    assert bad_guard == 0, "%s: %d bytes outside the rows written" % (
        what, bad_guard)
    assert bad_px == 0, "%s: %d pixel bytes differ" % (what, bad_px)


def call(lib, handle, r, sptr, dptr, stream=None):
    sw, sh, nw, nh = r["geom"]
    p = params(r)
    return lib.avirhip_lancir_resize_planes(
        handle, C.c_void_p(sptr), abi.MEM_DEVICE, sw, sh, C.c_void_p(dptr),
        abi.MEM_DEVICE, nw, nh, r["planes"], side(r, "src")[3],
        side(r, "dst")[3], C.byref(p), T[r["tin"]][0], T[r["tout"]][0], stream)
