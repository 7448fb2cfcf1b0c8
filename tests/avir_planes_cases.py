"""The case table of tests/test_gpu_avir_planes.py (CImageResizer over
single-channel planes: avirhip_resizer_resize_planes, k_avirp of
avir_amd/csrc/avirp.hip) and what its host-only check,
tests/test_avir_planes_table.py, needs to read it.

A row is one call: `planes` planes of one geometry (sw, sh, nw, nh), element
types `tin` / `tout` (names of tests/planes_cases.py's T), ResBitDepth `bits`,
resizing step `k` and offsets `ox`, `oy`, laid out with `gap` elements of
padding behind every plane on both sides (0: the call passes plane strides of
0, tightly packed), source rows `spad` elements longer than their pixels
(SrcScanlineSize; result rows are tight), the source base `soff` bytes off its
natural alignment, `far`: a plane stride in BYTES on both sides instead of
`gap`. `gamma`, `errd`, `fp4` choose the stages the kernel declines. `cls` is
the row's class: what the planner answers for it with one channel (steps()),
which the table test asserts, so that no row drifts out of its class. `road`
is the line the call has to print under AVIRHIP_VERBOSE: "k_avirp", "fallback"
for the classes the kernel declines, None where the LDS formula decides
(road()).

Expected bits: the reference's CImageResizer (tests/helpers.py, checker_avir)
on each plane as an (H, W, 1) image; half / bfloat16 as tests/dnf16_cases.py
defines them (the float32 call on the exactly widened source, narrowed to
nearest even). Layout, guard bytes and the byte-for-byte comparison are
tests/planes_cases.py's.

The seam rows follow the kernel's first tile (AP_TW x AP_TR output pixels),
read out of avirp.hip; lds_of() restates avirp.hip's range algebra and LDS
formula from the same file's constants."""
import ctypes as C
import os
import re
import numpy as np
from avir_amd import abi
from tests import helpers as H
from tests import dnf16_cases as D16
from tests import lancgp16_cases as L16
from tests import planes_cases as PC

T = PC.T
GUARD, FRONT = PC.GUARD, PC.FRONT
CSRC = PC.CSRC
DISTINCT = 6   # distinct source planes of a geometry; more repeat cyclically


def parse_constants(csrc=CSRC):
    """AP_TW, AP_TR, AP_RC, AP_LDS_PREF, AP_LDS_MAX, AP_MAXOPS and the candidate
    tiles (CAND) as avirp.hip defines them."""
    text = open(os.path.join(csrc, "avirp.hip")).read()
    out = {}
    for name in ("AP_TW", "AP_TR", "AP_RC", "AP_LDS_PREF", "AP_LDS_MAX",
                 "AP_MAXOPS", "AP_MAX_PIXELS"):
        m = re.search(r"^#define %s (\d+)\b" % name, text, re.M)
        assert m, "avirp.hip: no #define %s" % name
        out[name] = int(m.group(1))
    m = re.search(r"ap_cand\[\]\[ 2 \] = \{\{ AP_TW, AP_TR \}((?:,\s*\{ \d+, "
                  r"\d+ \})*)\};", text)
    assert m, "avirp.hip: no ap_cand"
    out["CAND"] = [(out["AP_TW"], out["AP_TR"])] + [
        (int(a), int(b)) for a, b in re.findall(r"\{ (\d+), (\d+) \}",
                                                m.group(1))]
    return out


K = parse_constants()
TW, TR = K["AP_TW"], K["AP_TR"]

# ---- geometries and their classes (H axis | V axis) ---------------------------
UPF = "FIR7 UP_FILTERED RESIZE(18)"
ZS = "FIR7 UP_ZEROSTUFF RESIZE2(24)"
GEOMS = {
    "upf_both": ((37, 23, 61, 40), UPF + " | " + UPF),
    "upf_2x": ((37, 23, 74, 46), UPF + " | " + UPF),
    "upf_h_zs_v": ((160, 120, 256, 192), UPF + " | " + ZS),
    "zs_both": ((320, 240, 512, 384), ZS + " | " + ZS),
    "zs_2x": ((224, 224, 448, 448), ZS + " | " + ZS),
    "dn_zs": ((96, 72, 64, 48), "UP_ZEROSTUFF RESIZE2(38) FIR7 | "
              "UP_ZEROSTUFF RESIZE2(38) FIR7"),
    "dn_near1": ((64, 48, 63, 47), "UP_ZEROSTUFF RESIZE2(26) FIR7 | "
                 "UP_ZEROSTUFF RESIZE2(26) FIR7"),
    "dn_fir_first": ((96, 72, 48, 36), "FIR7 RESIZE(18) FIR7 | "
                     "FIR7 RESIZE(18) FIR7"),
    "dn_fir_first20": ((130, 100, 64, 48), "FIR7 RESIZE(20) FIR7 | "
                       "FIR7 RESIZE(20) FIR7"),
    "dn3": ((96, 72, 32, 24), "RESIZE(38) FIR7 | RESIZE(38) FIR7"),
    "dn27": ((100, 80, 37, 30), "RESIZE(36) FIR7 | RESIZE(34) FIR7"),
    "dn_rf2": ((200, 150, 40, 30), "FIR19/2 RESIZE(24) FIR7 | "
               "FIR19/2 RESIZE(24) FIR7"),
    "dn_rf4": ((300, 200, 37, 25), None),
    "dn_rf8": ((400, 300, 25, 19), None),
    "mix_du": ((21, 33, 13, 70), None),
    "mix_ud": ((66, 40, 99, 27), None),
    "tiny": ((9, 7, 6, 5), None),
    "long_kernel": ((1100, 60, 64, 20), None),
}
# what the rows with `None` above must show instead of a whole signature
FIRST_FIR = {"dn_rf4": ((4, 31), (4, 31)), "dn_rf8": ((8, 61), (7, 59)),
             "long_kernel": ((8, 65), None)}

SEAM_UP, SEAM_DN = (50, 20), (140, 80)
SEAM_W = [TW - 1, TW, TW + 1, 2 * TW + 1]
SEAM_H = [TR - 1, TR, TR + 1, 2 * TR + 1]

PAIRS = [("u8", "u8"), ("u8", "f32"), ("u8", "u16"), ("u16", "u16"),
         ("u16", "u8"), ("f32", "f32"), ("f32", "u8"), ("f16", "f16"),
         ("bf16", "bf16"), ("f32", "f16"), ("f16", "f32")]
TYPE_GEOMS = ["upf_both", "dn3"]

ROWS = []


def _row(name, geom, tin="u8", tout="u8", planes=3, road="k_avirp", **kw):
    r = dict(name=name, geom=GEOMS[geom][0] if geom in GEOMS else geom,
             cls=geom if geom in GEOMS else None, tin=tin, tout=tout,
             planes=planes, road=road, bits=None, k=0.0, ox=0.0, oy=0.0, gap=0,
             spad=0, soff=0, far=0, gamma=False, errd=False, fp4=False)
    assert set(kw) <= set(r), kw
    r.update(kw)
    if r["bits"] is None:
        r["bits"] = 8 if tout == "u8" else 16
    ROWS.append(r)


# ---- class by class
for _g in GEOMS:
    if _g not in ("dn_rf8", "long_kernel"):
        _row(_g, _g)
_row("dn_rf8", "dn_rf8", planes=2, road=None)   # (decided by lds_of below)
_row("long_kernel", "long_kernel", planes=2, road=None)
CLASS_ROWS = list(GEOMS)

# ---- tile seams
SEAM_ROWS = []
for _w in SEAM_W:
    for _h in SEAM_H:
        for _t, _s in (("up", SEAM_UP), ("dn", SEAM_DN)):
            _row("seam_%s_%dx%d" % (_t, _w, _h), _s + (_w, _h), planes=2)
            SEAM_ROWS.append(ROWS[-1]["name"])

# ---- crop: explicit k, ox, oy
_row("crop_zs", "zs_both", planes=2, k=0.7, ox=12.25, oy=7.5)
_row("crop_upf", "upf_both", planes=2, k=0.55, ox=2.25, oy=1.5)
_row("crop_dn", "dn3", planes=2, k=2.5, ox=3.75, oy=-1.25)

# ---- element types
for _g in TYPE_GEOMS:
    for _a, _b in PAIRS:
        _row("type_%s_%s_%s" % (_g, _a, _b), _g, _a, _b, planes=2)
_row("res16_u16", "upf_both", "u16", "u16", planes=2, bits=16)
_row("res16_u16_dn", "dn3", "u8", "u16", planes=2, bits=16)
_row("trunc_u8", "dn3", "u8", "u8", planes=2, bits=6)
_row("trunc_f32_u8", "upf_both", "f32", "u8", planes=2, bits=5)

# ---- plane counts and strides
for _n in (1, 3, 5, 6):
    _row("planes%d_packed" % _n, "upf_both", planes=_n)
_row("planes3_gap7", "upf_both", planes=3, gap=7)
_row("planes5_gap7_dn", "dn27", planes=5, gap=7)
_row("scanline_pad", "upf_both", planes=3, spad=3)
_row("scanline_pad_gap", "dn_zs", "u16", "u16", planes=2, spad=5, gap=7)
_row("far_planes", "upf_both", planes=2, far=2 ** 31 + 64)
_row("many_planes", "tiny", planes=70000)

# ---- the measured threshold (AP_MAX_PIXELS source or result pixels a plane):
# a row on each side of it
_row("px_at", (512, 512, 320, 320), planes=2)
_row("px_above", (520, 512, 320, 320), planes=2, road="fallback")

# ---- the classes avirp_run declines
_row("f64", "upf_both", "f64", "f64", planes=2, road="fallback")
_row("odd_base", "upf_both", "f16", "f16", planes=2, soff=1, road="fallback")
_row("gamma_u8", "upf_both", planes=2, gamma=True, road="fallback")
_row("errd_u8", "upf_both", planes=2, errd=True, road="fallback")
_row("fp4", "upf_both", "f32", "f32", planes=2, fp4=True, road="fallback")

NAMES = [r["name"] for r in ROWS]
FALLBACK_MAY = ["long_kernel", "f64", "odd_base", "gamma_u8", "errd_u8", "fp4"]
DECLINED = ["px_above"]    # by measurement (avirp.hip, AP_MAX_PIXELS)
CROSS = ["upf_both", "dn3", "type_upf_both_f16_f16"]
STREAM_ROW, NUMPY_ROW = "dn_zs", "mix_ud"


def row(name):
    return ROWS[NAMES.index(name)]


# ---- the planner's answer (host only) -----------------------------------------

class desc(object):
    """with desc(r) as d: the plan description of the row with one channel."""

    def __init__(self, r):
        self.r = r

    def __enter__(self):
        r = self.r
        sw, sh, nw, nh = r["geom"]
        tin = "f32" if r["tin"] in ("f16", "bf16") else r["tin"]
        tout = "f32" if r["tout"] in ("f16", "bf16") else r["tout"]
        self.h, self.d = H.product_desc(
            sw, sh, nw, nh, 1, k=r["k"], in_type=T[tin][0],
            out_type=T[tout][0], resbits=r["bits"], ox=r["ox"], oy=r["oy"],
            sstride=sw + r["spad"] if r["spad"] else 0,
            fpclass=4 if r["fp4"] else 1)
        return self.d.contents

    def __exit__(self, *a):
        H.free_product_desc(self.h, self.d)
        return False


def _sig(s):
    if s.kind == abi.STEP_FIR:
        return "FIR%d" % s.flt_len + ("/%d" % s.resample_factor
                                      if s.resample_factor > 1 else "")
    if s.kind in (abi.STEP_RESIZE, abi.STEP_RESIZE2):
        return "%s(%d)" % (abi.STEP_NAMES[s.kind], s.bank_filter_len)
    return abi.STEP_NAMES[s.kind]


def steps(r):
    """"<H axis> | <V axis>": the kinds of the steps, a FIR with its length
    (and /factor where it decimates), a resizing step with its bank length."""
    with desc(r) as d:
        return " | ".join(" ".join(_sig(a.steps[i]) for i in range(a.n_steps))
                          for a in (d.h, d.v))


def first_fir(r):
    """((rf, taps) of the H axis' first step, of the V axis'), None where
    that is no FIR."""
    with desc(r) as d:
        out = []
        for a in (d.h, d.v):
            s = a.steps[0]
            out.append((s.resample_factor, s.flt_len)
                       if s.kind == abi.STEP_FIR else None)
        return tuple(out)


# ---- avirp.hip's range algebra and LDS formula, restated -----------------------

def lower(ax):
    """The ops of an axis as api.cpp lower_axis makes them, as dicts."""
    ops, zs, prev = [], None, None
    for i in range(ax.n_steps):
        s = ax.steps[i]
        op = dict(view="raw" if prev else "clamp", in_len=s.in_len,
                  in_prefix=prev["out_prefix"] if prev else 0,
                  out_len=s.out_len)
        if s.kind == abi.STEP_FIR:
            op.update(type="fir", rf=s.resample_factor, lat=s.flt_latency,
                      e=s.edge_pixel_count)
        elif s.kind == abi.STEP_UP_ZEROSTUFF:
            zs = s
            continue
        elif s.kind == abi.STEP_UP_FILTERED:
            op.update(type="upf", view="clamp", rf=s.resample_factor,
                      flen=s.flt_len, up_inprefix=s.in_prefix,
                      up_R=s.in_prefix + s.in_len + s.in_suffix,
                      sdc_len=s.suffix_dc_len, pdc_len=s.prefix_dc_len,
                      pdc_d0=s.out_prefix - s.in_prefix * s.resample_factor,
                      out_prefix=s.out_prefix,
                      out_total=s.out_prefix + s.out_len + s.out_suffix)
        else:
            r = np.ctypeslib.as_array(s.rpos, shape=(s.out_len,))
            stp = 2 if zs is not None else 1
            start = r["src_offs_px"].astype(np.int64) // stp
            nt = (r["fl"].astype(np.int64) + stp - 1) // stp
            op.update(type="gather", start=start, end=start + nt - 1)
            if zs is not None:
                op.update(view="zs", in_len=zs.in_len)
                zs = None
        ops.append(op)
        prev = op if op["type"] == "upf" else None
    return ops


def _need(op, a, b):
    """ap_need of avirp.hip: stored indices of the input for stored indices
    [a, b] of the output."""
    n = op["in_len"]
    if op["type"] == "upf":
        rf = op["rf"]
        rlo = a - op["flen"] + 1
        rlo = 0 if rlo <= 0 else (rlo + rf - 1) // rf
        rhi = min(b // rf, op["up_R"] - 1)
        lo, hi = 1 << 30, -(1 << 30)
        if rlo <= rhi:
            lo = max(0, min(rlo - op["up_inprefix"], n - 1))
            hi = max(0, min(rhi - op["up_inprefix"], n - 1))
        if (op["sdc_len"] > 0 and b >= op["up_R"] * rf and
                a < op["up_R"] * rf + op["sdc_len"]):
            lo, hi = min(lo, n - 1), max(hi, n - 1)
        if (op["pdc_len"] > 0 and b >= op["pdc_d0"] and
                a < op["pdc_d0"] + op["pdc_len"]):
            lo, hi = min(lo, 0), max(hi, 0)
        return (0, 0) if lo > hi else (lo, hi)
    if op["type"] == "fir":
        ia = op["rf"] * (a - op["e"]) - op["lat"]
        ib = op["rf"] * (b - op["e"]) + op["lat"]
    else:
        ia = int(op["start"][a:b + 1].min())
        ib = int(op["end"][a:b + 1].max())
    if op["view"] == "raw":
        return ia + op["in_prefix"], ib + op["in_prefix"]
    return max(0, min(ia, n - 1)), max(0, min(ib, n - 1))


def axis_counts(ops, dst_len, t):
    """Per buffer 0 .. len(ops): the largest count a tile of `t` outputs
    needs (ap_ranges' maxn)."""
    mx = [0] * (len(ops) + 1)
    for a0 in range(0, dst_len, t):
        a, b = a0, min(a0 + t, dst_len) - 1
        mx[len(ops)] = max(mx[len(ops)], b - a + 1)
        for i in range(len(ops) - 1, -1, -1):
            a, b = _need(ops[i], a, b)
            mx[i] = max(mx[i], b - a + 1)
    return mx


def lds_of(r, tile=None):
    """(bytes of LDS, tile) avirp_run's rule gives the row: the first
    candidate within AP_LDS_PREF, else the first within AP_LDS_MAX; (None,
    None) where there is none, or an axis has more than AP_MAXOPS ops."""
    with desc(r) as d:
        oh, ov = lower(d.h), lower(d.v)
        nw, nh = d.new_w, d.new_h
    if max(len(oh), len(ov)) > K["AP_MAXOPS"]:
        return None, None
    best = (None, None)
    for tw, tr in ([tile] if tile else K["CAND"]):
        hm, vm = axis_counts(oh, nw, tw), axis_counts(ov, nh, tr)
        reg = [0, 0, vm[0] * tw]
        rc = min(vm[0], K["AP_RC"])
        for s in range(len(oh)):
            reg[s & 1] = max(reg[s & 1], rc * hm[s])
        for i in range(1, len(ov)):
            reg[(i - 1) & 1] = max(reg[(i - 1) & 1], vm[i] * tw)
        lds = 4 * sum(reg)
        if lds <= K["AP_LDS_PREF"]:
            return lds, (tw, tr)
        if best[0] is None and lds <= K["AP_LDS_MAX"]:
            best = (lds, (tw, tr))
    return best


def pixels(r):
    sw, sh, nw, nh = r["geom"]
    return max(sw * sh, nw * nh)


def road(r):
    if r["road"] is not None:
        return r["road"]
    if pixels(r) > K["AP_MAX_PIXELS"]:
        return "fallback"
    return "k_avirp" if lds_of(r)[0] is not None else "fallback"


# ---- inputs and expected bits ---------------------------------------------------

_SRC, _REF = {}, {}


def _rt(tout):
    return tout if tout in ("u8", "u16", "f64") else "f32"


def sources(r):
    """(DISTINCT, sh, sw) source planes of the row's type, shared; plane i of
    a call is plane i % DISTINCT of them."""
    sw, sh = r["geom"][:2]
    key = (sw, sh, r["tin"])
    if key not in _SRC:
        if r["tin"] == "f64":
            a = L16.source((DISTINCT, sh, sw), "f32",
                           seed=sw + sh).astype(np.float64)
        else:
            a = L16.source((DISTINCT, sh, sw), r["tin"], seed=sw + sh + 1)
        a.setflags(write=False)
        _SRC[key] = a
    return _SRC[key]


def source_planes(r):
    s = sources(r)
    return [s[i % DISTINCT] for i in range(r["planes"])]


def reference(r, i):
    """The reference's result for source plane `i` (< DISTINCT) in elements
    of the result's class (float32, uint8, uint16, float64), once per distinct
    call."""
    rt = _rt(r["tout"])
    key = (r["geom"], r["tin"], rt, r["bits"], r["k"], r["ox"], r["oy"],
           r["gamma"], r["errd"], r["fp4"], i)
    if key not in _REF:
        sw, sh, nw, nh = r["geom"]
        src = sources(r)[i].reshape(sh, sw, 1)
        kw = dict(k=r["k"], out_dtype=T[rt][1], resbits=r["bits"], ox=r["ox"],
                  oy=r["oy"])
        if r["gamma"]:
            kw["gamma"] = True
        if r["errd"]:
            kw["errd"] = True
        if r["fp4"]:
            kw["variant"] = 1
        ref = H.checker_avir(np.ascontiguousarray(
            L16.ref_input(src, r["tin"])), nw, nh, **kw)
        ref = np.ascontiguousarray(ref).reshape(nh, nw)
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def expected(r, i):
    return D16.from_f32(reference(r, i % DISTINCT), r["tout"])


# ---- layout (tests/planes_cases.py's, result rows tight) ------------------------

def _lay(r):
    return dict(r, npad=0)


def side(r, which):
    return PC.side(_lay(r), which)


def regions(r, which, planes):
    """As planes_cases.regions; tightly packed planes in one piece (the
    70,000-plane row)."""
    w, h, pitch, _, stride, es = side(r, which)
    if planes is not None and not r["far"] and pitch == w and stride == h * w:
        body = np.concatenate([np.ascontiguousarray(p).view(np.uint8).ravel()
                               for p in planes])
        g = np.full(FRONT, GUARD, np.uint8)
        return [(-FRONT, np.concatenate([g, body, g]))]
    return PC.regions(_lay(r), which, planes)


def device_side(r, which, planes):
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
    return PC.read_back(_lay(r), t)


def compare(r, got, what):
    """Byte for byte against the expected image: pixels and guards."""
    exp = [expected(r, i) for i in range(min(r["planes"], DISTINCT))]
    exp = [exp[i % DISTINCT] for i in range(r["planes"])]
    want = regions(r, "dst", exp)
    mask = regions(r, "dst", [np.zeros_like(e) for e in exp])
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


# ---- the call ---------------------------------------------------------------------

def resizer(lib, r):
    """A resizer object of the row's kind (the caller destroys it)."""
    h = C.c_void_p()
    abi.check(lib.avirhip_resizer_create(r["bits"], 0, None, C.byref(h)),
              "resizer_create")
    if r["errd"]:
        abi.check(lib.avirhip_resizer_set_ditherer(h, abi.DITHER_ERRD),
                  "set_ditherer")
    if r["fp4"]:
        abi.check(lib.avirhip_resizer_set_fpclass(h, 4), "set_fpclass")
    return h


def vars_of(r):
    v = abi.Vars()
    abi.load().avirhip_vars_default(C.byref(v))
    v.ox, v.oy = r["ox"], r["oy"]
    v.UseSRGBGamma = 1 if r["gamma"] else 0
    return v


def call(lib, handle, r, sptr, dptr, stream=None, mem=abi.MEM_DEVICE):
    sw, sh, nw, nh = r["geom"]
    v = vars_of(r)
    return lib.avirhip_resizer_resize_planes(
        handle, C.c_void_p(sptr), mem, sw, sh,
        sw + r["spad"] if r["spad"] else 0, C.c_void_p(dptr), mem, nw, nh,
        r["planes"], side(r, "src")[3], side(r, "dst")[3], float(r["k"]),
        C.byref(v), T[r["tin"]][0], T[r["tout"]][0], stream)
