"""Rows that lie 2 GiB and 4 GiB from the image's base, on every kernel
family (tests/far_row_cases.py: the families' own limits and the row pitches
on either side of them).

Per row and level the packed image is resized by the reference
(tests/helpers.py: checker_avir / checker_lancir, as everywhere in the suite);
the device holds the same rows `pitch` elements apart in a buffer of 0xFF
bytes (a NaN for every float type) which the host never sees. The calls: the
whole frame, the three bands of gpass_route_cases.bands, a band of the last
output rows alone (its source rows are the far ones) and, where the family
reads a device window where it lies, avirhip_resize_window of those last rows:
the kernel then sees a virtual base 2 or 4 GiB below the pointer it was given.

Raw words are compared; a NaN only has to be a NaN.
  automatic path, every level        rc == 0, 0 differing words
  forced path, inside the limit      the same -- a refusal fails the test
  forced path, outside a host guard  0 differing words, or
                                     AVIRHIP_EUNSUPPORTED with the destination
                                     untouched
  no guard (64-bit addresses)        the forced path runs at every level
  CLancIR destination levels         the written region equals the reference,
                                     the padding still holds the fill
Wrong pixels with rc == 0 is the failure this file exists for. That an
`under` case runs the kernels its row is named after is not something rc
shows: profiles/far_rows/ (tools/gpass_route_trace.py --far)."""
import ctypes as C
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import far_row_cases as F
from tests import gpass_route_cases as G
from tests import helpers as H
from tests import refbind as rb

pytestmark = pytest.mark.gpu

FILL = 0xFF
LAST = 3          # output rows of the band of the last rows
BF16_NAN = 0x7fc0


def _narrow_bf16(f):
    """float32 -> bfloat16 bits, round to nearest even (include/avirhip.h)."""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[np.isnan(f)] = BF16_NAN
    return r


def _widen_bf16(b):
    return (np.ascontiguousarray(b).astype(np.uint32) << 16).view(np.float32)


def _image(r, sh):
    """The packed source of a row, (sh, sw, ch), in its host type."""
    sw, ch, t = r["sw"], r["ch"], r["tin"]
    if t in ("u8", "u16"):
        n = F.TYPES[t][2]
        raw = rb.lcg_u8((sh, sw, ch, n), seed=sw + ch)
        return np.ascontiguousarray(raw).view(F.TYPES[t][1]).reshape(
            sh, sw, ch)
    a = rb.lcg_f32((sh, sw, ch), seed=7 * sw + ch)
    if t == "f64":
        b = rb.lcg_f32((sh, sw, ch), seed=sh)
        return a.astype(np.float64) + b.astype(np.float64) * 2.0 ** -25
    if t == "f16":
        return a.astype(np.float16)
    return _narrow_bf16(a) if t == "bf16" else a


_wants = {}


def _want(r, sh):
    """The reference's result of the packed image: computed once per row and
    height, shared by the levels and left unchanged."""
    key = (r["name"] if r["by"] == "rows" else
           (r["fe"], r["sw"], r["sh"], r["nw"], r["nh"], r["ch"], r["tin"],
            r["tout"], tuple(sorted(r["ex"].items()))), sh)
    if key in _wants:
        return _wants[key]
    img = _image(r, sh)
    nw, nh = r["nw"], (2 * sh if r["by"] == "rows" else r["nh"])
    tin, tout = r["tin"], r["tout"]
    if tin in ("f16", "bf16"):
        # (include/avirhip.h: the float32 call, its result narrowed)
        f = _widen_bf16(img) if tin == "bf16" else img.astype(np.float32)
        res = H.checker_avir(f, nw, nh, out_dtype=np.float32,
                             resbits=r["bits"], threads=8)
        with np.errstate(over="ignore", invalid="ignore"):
            want = (_narrow_bf16(res) if tout == "bf16" else
                    res.astype(np.float16))
    elif r["fe"] == "lancir":
        want = H.checker_lancir(img, nw, nh, out_dtype=F.TYPES[tout][1])
    else:
        kw = {}
        if r["ex"].get("fp") == abi.FPCLASS_DOUBLE:
            assert H.need_ref("the double class")
            kw["variant"] = 4
        want = H.checker_avir(img, nw, nh, out_dtype=F.TYPES[tout][1],
                              resbits=r["bits"], threads=8,
                              build_mode=r["ex"].get("build_mode", -1), **kw)
    want.setflags(write=False)
    img.setflags(write=False)
    _wants[key] = (img, want)
    return _wants[key]


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32,
                   8: np.uint64}[a.dtype.itemsize])


def _isnan(a, t):
    if t == "bf16":
        return np.isnan(_widen_bf16(a))
    return np.isnan(a) if a.dtype.kind == "f" else np.zeros(a.shape, bool)


def _differ(got, want, tout):
    """Differing raw words; NaN == NaN whatever the payload."""
    got = np.ascontiguousarray(got).view(want.dtype).reshape(want.shape)
    bad = _words(got) != _words(want)
    bad &= ~(_isnan(got, tout) & _isnan(want, tout))
    return int(bad.sum())


def _plan(r, lv, path):
    """-> (front end: keeps the plan alive, plan or None when set_path
    refused the path with AVIRHIP_EUNSUPPORTED)."""
    lib = abi.load()
    obj, arg = F.front_end(r, lv)
    c = F.case(r, lv)
    fe, sw, sh, nw, nh, ch = c[:6]
    ti, to = F.TYPES[r["tin"]][0], F.TYPES[r["tout"]][0]
    if fe == "lancir":
        p = obj.plan(sw, sh, nw, nh, ch, arg, ti, to)
    else:
        p = obj.plan(sw, sh, nw, nh, ch, 0.0, arg, ti, to,
                     lv.pitch if r["by"] != "dst" else 0)
    rc = lib.avirhip_plan_set_path(p, path)
    if rc != 0:
        assert rc == abi.EUNSUPPORTED, (rc, lib.avirhip_last_error())
        return obj, None
    abi.check(lib.avirhip_plan_set_variant(p, r["variant"] if path else 0),
              "set_variant")
    return obj, p


class _Pitched(object):
    """A device buffer of FILL bytes with `rows` rows of row_b bytes lying
    pitch_b apart; `view` is the (rows, pitch_b) strided view of it (the last
    row ends with its pixels, as the allocation does)."""

    def __init__(self, rows, row_b, pitch_b):
        import torch
        self.rows, self.row_b, self.pitch_b = rows, row_b, pitch_b
        n = (rows - 1) * pitch_b + row_b
        assert n + 256 <= F.CAP
        self.buf = torch.full((n + 256,), FILL, dtype=torch.uint8,
                              device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0
        self.img = torch.as_strided(self.buf, (rows, row_b), (pitch_b, 1))

    def ptr(self, row=0):
        return self.buf.data_ptr() + row * self.pitch_b

    def put(self, packed):
        """The packed host image (rows, ...) into the rows."""
        import torch
        a = np.ascontiguousarray(packed).view(np.uint8).reshape(
            self.rows, self.row_b)
        self.img.copy_(torch.from_numpy(a).to("cuda:0"))

    def rows_of(self, a, b):
        return self.img[a:b].contiguous().cpu().numpy()

    def padding_holds(self):
        """Every byte between the rows still is FILL: compared on the device,
        a few rows at a time."""
        import torch
        pad = torch.as_strided(self.buf, (self.rows - 1,
                                          self.pitch_b - self.row_b),
                               (self.pitch_b, 1), self.row_b)
        step = max(1, (256 << 20) // max(1, self.pitch_b))
        for i in range(0, self.rows - 1, step):
            if not bool((pad[i:i + step] == FILL).all()):
                return False
        return bool((self.buf[-256:] == FILL).all())


def _calls(r, lv, lib, p, src, want, what, native):
    """The calls of one plan -> (calls that ran, calls refused, problems)."""
    import torch
    nh, nw, ch = want.shape
    osz = F.TYPES[r["tout"]][2]
    rowb = nw * ch * osz
    dst_mode = (r["by"] == "dst")
    todo = [("frame", [(0, nh)]), ("bands", G.bands(nh)),
            ("last", [(nh - LAST, nh)])]
    ran = refused = 0
    problems = []
    if dst_mode:
        dst = _Pitched(nh, rowb, lv.pitch * osz)
    for how, bands in todo + ([("window", [(nh - LAST, nh)])]
                              if native else []):
        if dst_mode:
            dst.img.fill_(FILL)
        else:
            d = torch.zeros(nh * rowb + 64, dtype=torch.uint8,
                            device="cuda:0")
        rcs = []
        for (a, b) in bands:
            dp = dst.ptr(a) if dst_mode else d.data_ptr() + a * rowb
            if how == "window":
                fa, fb = C.c_int(), C.c_int()
                abi.check(lib.avirhip_band_source_rows(
                    p, a, b, C.byref(fa), C.byref(fb)), "band_source_rows")
                rcs.append(lib.avirhip_resize_window(
                    p, C.c_void_p(src.ptr(fa.value)), abi.MEM_DEVICE,
                    fa.value, fb.value - fa.value + 1, C.c_void_p(dp),
                    abi.MEM_DEVICE, a, b, None))
            else:
                rcs.append(lib.avirhip_resize_band(
                    p, C.c_void_p(src.ptr()), abi.MEM_DEVICE, C.c_void_p(dp),
                    abi.MEM_DEVICE, a, b, None))
        torch.cuda.synchronize()
        for (a, b), rc in zip(bands, rcs):
            got = (dst.rows_of(a, b) if dst_mode else
                   d[a * rowb:b * rowb].cpu().numpy())
            tag = "%s %s rows [%d, %d)" % (what, how, a, b)
            if rc == abi.EUNSUPPORTED:
                refused += 1
                clean = (got == (FILL if dst_mode else 0)).all()
                print("%s: refused (%s)" % (
                    tag, lib.avirhip_last_error().decode()))
                if not clean:
                    problems.append("%s: a refused call wrote its "
                                    "destination" % tag)
                continue
            if rc != 0:
                problems.append("%s: rc %d %r" % (
                    tag, rc, lib.avirhip_last_error()))
                continue
            ran += 1
            nd = _differ(got, want[a:b], r["tout"])
            print("%s: %d of %d words differ" % (tag, nd, want[a:b].size))
            if nd:
                problems.append("%s: %d of %d words differ with rc == 0" % (
                    tag, nd, want[a:b].size))
        if dst_mode and not dst.padding_holds():
            problems.append("%s %s: the destination's padding was written"
                            % (what, how))
        if not dst_mode:
            del d
    return ran, refused, problems


def _run_level(r, lv):
    """One row at one level: the forced path, then the automatic one.
    -> (the forced path ran every call, problems)"""
    import torch
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    img, want = _want(r, lv.sh)
    isz = F.TYPES[r["tin"]][2]
    row_b = r["sw"] * r["ch"] * isz
    src = _Pitched(lv.sh, row_b,
                   row_b if r["by"] == "dst" else lv.pitch * isz)
    src.put(img)
    must = lv.inside or not r["limit"]["guard"]
    problems = []
    forced_ran = False
    with G.environment(r["env"]):
        for path in ([r["path"]] if r["path"] else []) + [0]:
            forced = (path != 0 or r["path"] == 0)
            what = "%s %s (%s %d, pitch %d) path %d" % (
                r["name"], lv.name, "rows" if r["by"] == "rows" else "row",
                lv.sh, lv.pitch, path)
            obj, p = _plan(r, lv, path)
            if p is None:
                print("%s: set_path refused" % what)
                if must or path == 0:
                    problems.append("%s: set_path refused inside the limit"
                                    % what)
                continue
            run_path = lib.avirhip_plan_get_path(p)
            native = bool(r["window"] and must and run_path == 4)
            ran, refused, pr = _calls(r, lv, lib, p, src, want, what, native)
            print("%s: runs path %d, %d calls ran, %d refused, plan holds "
                  "%d bytes" % (what, run_path, ran, refused,
                                lib.avirhip_plan_device_bytes(p)))
            problems += pr
            if refused and (must or path == 0):
                problems.append("%s: %d calls refused %s" % (
                    what, refused, "on the automatic path" if path == 0
                    else "inside the limit"))
            if forced and path == r["path"] and refused == 0 and not pr:
                forced_ran = True
            del obj, p
    del src
    torch.cuda.empty_cache()
    return forced_ran, problems


@pytest.mark.parametrize("level", F.LEVELS)
@pytest.mark.parametrize("group", F.GROUPS)
def test_far_rows(group, level):
    rows = F.group(group)
    problems = []
    ran = floor = 0
    for r in rows:
        lv = F.level(r, level)
        if lv.dropped:
            print("%s %s: dropped, %s" % (r["name"], level, lv.dropped))
            continue
        must = lv.inside or not r["limit"]["guard"]
        floor += must
        ok, pr = _run_level(r, lv)
        problems += pr
        ran += (ok and must)
    assert not problems, "\n".join(problems)
    # the floor: every row of the group whose level has to run on its forced
    # path did run there, every call of it (a condition, not a measurement;
    # at `under` that is every row the memory cap does not drop)
    print("%s %s: %d forced-path cases ran, the floor is %d" % (
        group, level, ran, floor))
    assert ran >= floor, (ran, floor)
    if level == "under":
        assert floor == sum(1 for r in rows
                            if not F.level(r, "under").dropped)
