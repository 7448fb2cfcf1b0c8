"""Every kernel family at every byte alignment of its images
(tests/align_cases.py: what each family's fast road asks of the caller's
bases and pitches, as its launcher states it, and the levels on either side).

Per row the packed image of each geometry is resized once by the reference
(tests/helpers.py: checker_avir / checker_lancir, through
tests/test_gpu_far_rows.py's _want); the device calls go through
avirhip_resize_band / avirhip_resize_window on torch byte tensors. The source
lies `soff` bytes into an allocation that ends with the image's last element,
its row padding filled as tests/test_gpu_window.py fills it; the destination
lies 16 + `doff` bytes into an allocation of sentinel bytes with a row and 16
bytes behind the image.

  every level, forced path   rc == 0 and 0 differing raw words; every byte
                             outside the stored span, and between CLancIR's
                             rows, still holds the sentinel
  a level on the fast road   the family's AVIRHIP_VERBOSE line is there, the
                             pack pass' and the output stage's are not (beyond
                             those of the aligned call)
  a level the table places   the side's `tell` shows: the stage's line; or the
  aside                      forced path refuses (AVIRHIP_EUNSUPPORTED, the
                             destination untouched) and the automatic path
                             serves the same pointers with the reference's bits
A fast level that quietly stepped aside fails, and so does an aside level that
ran the fast road. Problems are collected per row and asserted once."""
import ctypes as C
import re
import numpy as np
import pytest
from avir_amd import abi
from tests import align_cases as A
from tests import gpass_route_cases as G
from tests import window_cases as W
from tests import helpers as H
from tests.test_gpu_far_rows import _want, _differ, _image
from tests.test_gpu_gp16 import _dev
from tests.test_gpu_window import _dev_sentinel, _flat, SENTINEL

pytestmark = pytest.mark.gpu

FRONT = 16
TAG = re.compile(r"^(k_\w+|pack pass|output stage):", re.M)
STAGE = {"pack pass": "pack", "output stage": "out"}


def _tags(err):
    return set(TAG.findall(err))


def _stages(tags):
    return set(STAGE[t] for t in tags if t in STAGE)


def _ran(r, tags):
    """The family's kernel printed its line. Rows without one (`kernel` None:
    the per-op kernels, the tiles, tile64, generic64, CLancIR's double rows,
    the ditherer) have other evidence: a float RGBA row is refused on its
    forced path when it misses a modulus, and ran there when it was not; an
    integer row shows no `pack pass` line beyond the aligned call's (_road:
    seen - expect), and where the row pins `base` without "pack" that call
    shows none either -- the loaders read the caller's image raw."""
    return r["kernel"] is None or any(t.startswith(r["kernel"]) for t in tags)


_errd_wants = {}


def _reference(q):
    """(image, the reference's result) of a row at its geometry: far-row's
    _want, or for the ditherer the reference with its error-diffusion class."""
    if not q["ex"].get("errd"):
        return _want(q, q["sh"])
    key = (q["sw"], q["sh"], q["nw"], q["nh"], q["ch"], q["tin"])
    if key not in _errd_wants:
        img = _image(q, q["sh"])
        want = H.checker_avir(img, q["nw"], q["nh"],
                              out_dtype=A.TYPES[q["tout"]][1],
                              resbits=q["bits"], errd=True, threads=8)
        img.setflags(write=False)
        want.setflags(write=False)
        _errd_wants[key] = (img, want)
    return _errd_wants[key]


def _plan(r, lv, path):
    """-> (front end: keeps the plan alive, plan or None: set_path refused)."""
    lib = abi.load()
    obj, arg = A.front_end(r, lv)
    sw, sh, nw, nh = A.geom(r, lv.g)
    ti, to = A.TYPES[r["tin"]][0], A.TYPES[r["tout"]][0]
    sp, dp = A.pitches(r, lv)
    if r["fe"] == "lancir":
        p = obj.plan(sw, sh, nw, nh, r["ch"], arg, ti, to)
    else:
        p = obj.plan(sw, sh, nw, nh, r["ch"], 0.0, arg, ti, to,
                     sp if lv.spad else 0)
    rc = lib.avirhip_plan_set_path(p, path)
    if rc != 0:
        assert rc == abi.EUNSUPPORTED, (rc, lib.avirhip_last_error())
        return obj, None
    abi.check(lib.avirhip_plan_set_variant(p, r["variant"] if path else 0),
              "set_variant")
    return obj, p


def _source(r, lv, img):
    """The rows at the level's pitch, padding filled (test_gpu_window._flat)."""
    sp, dp = A.pitches(r, lv)
    fill = np.nan if img.dtype.kind == "f" else np.iinfo(img.dtype).max
    return _flat(img, sp, fill)


class _Dst(object):
    """The destination image 16 + doff bytes into sentinel bytes, rows dp_b
    apart, a row and 16 bytes behind it."""

    def __init__(self, r, lv, host=False):
        sw, sh, nw, nh = A.geom(r, lv.g)
        sp, dp = A.pitches(r, lv)
        ed = A.esz_out(r)
        self.nh, self.row_b, self.dp_b = nh, nw * r["ch"] * ed, dp * ed
        self.off = FRONT + lv.doff
        self.span = (nh - 1) * self.dp_b + self.row_b
        self.n = self.off + self.span + self.dp_b + 16
        assert self.n < A.CAP
        self.host = host
        if host:
            self.raw = np.full(self.n + 32, SENTINEL, np.uint8)
            self.skip = (-self.raw.ctypes.data) % 16
            self.base = self.raw.ctypes.data + self.skip
        else:
            self.t = _dev_sentinel(self.n)
            self.base = self.t.data_ptr()
        assert self.base % 16 == 0

    def ptr(self, row=0):
        return self.base + self.off + row * self.dp_b

    def bytes(self):
        import torch
        if self.host:
            return self.raw[self.skip:self.skip + self.n].copy()
        torch.cuda.synchronize()
        return self.t.cpu().numpy()

    def check(self, r, want, stored, what, problems, log):
        """Rows of `stored` [(a, b)] equal the reference's, every other byte
        is the sentinel."""
        g = self.bytes()
        mask = np.zeros(self.n, bool)
        for a, b in stored:
            rows = np.empty((b - a, self.row_b), np.uint8)
            for y in range(a, b):
                o = self.off + y * self.dp_b
                mask[o:o + self.row_b] = True
                rows[y - a] = g[o:o + self.row_b]
            nd = _differ(rows.reshape(-1), want[a:b], r["tout"])
            log.append("%s rows [%d, %d): %d of %d words differ" % (
                what, a, b, nd, want[a:b].size))
            if nd:
                w = np.ascontiguousarray(want[a:b]).view(np.uint8).reshape(-1)
                first = int(np.flatnonzero(rows.reshape(-1) != w)[0])
                problems.append("%s rows [%d, %d): %d of %d words differ, the "
                                "first in byte %d of the band" % (
                                    what, a, b, nd, want[a:b].size, first))
        out = np.flatnonzero((g != SENTINEL) & ~mask)
        if out.size:
            problems.append("%s: %d bytes outside the stored span were "
                            "written, the first %d bytes from the image's base"
                            % (what, out.size, int(out[0]) - self.off))


def _road(r, tags, base, tells, what, problems):
    """The road a forced call with rc == 0 took, against the table."""
    if not _ran(r, tags):
        problems.append("%s: no %s line (%r)" % (what, r["kernel"],
                                                 sorted(tags)))
    seen = _stages(tags) - base
    expect = set(t for t in tells if t in ("pack", "out"))
    if seen - expect:
        problems.append("%s: a level on the fast road stepped aside to %r"
                        % (what, sorted(seen - expect)))
    if expect - seen:
        problems.append("%s: the table places it aside (%r), the call showed "
                        "%r" % (what, sorted(expect), sorted(seen)))


def _run_row(r, capfd):
    import torch
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    problems, log = [], []
    wants = {}
    for g in ((0, 1) if r["geom2"] else (0,)):
        q = A.at(r, g)
        wants[g] = _reference(q)
        assert wants[g][1].shape == (q["nh"], q["nw"], r["ch"])
    plans, srcs = {}, {}

    def plan(lv, path):
        # (the window levels: a plan of their own, which has staged nothing)
        key = (lv.g, lv.spad, lv.dpad, path, lv.call == "window")
        if key not in plans:
            plans[key] = _plan(r, lv, path)
        return plans[key][1]

    def source(lv):
        key = (lv.g, lv.spad, lv.soff)
        if key not in srcs:
            flat = _source(r, lv, wants[lv.g][0])
            t = _dev(flat, off=lv.soff)
            assert t.data_ptr() % 16 == 0
            assert t.numel() == lv.soff + flat.nbytes  # (no tail at all)
            srcs[key] = t
        return srcs[key].data_ptr() + lv.soff

    def call(p, sptr, dptr, a, b, mem=abi.MEM_DEVICE):
        capfd.readouterr()
        rc = lib.avirhip_resize_band(p, C.c_void_p(sptr), mem,
                                     C.c_void_p(dptr), mem, a, b, None)
        msg = lib.avirhip_last_error()
        torch.cuda.synchronize()
        return rc, _tags(capfd.readouterr().err), msg

    base = None
    uses = set(s["tell"] for s in r["sides"].values()) & {"pack", "out"}
    for lv in A.levels(r):
        img, want = wants[lv.g]
        nh = want.shape[0]
        what = "%s %s" % (r["name"], lv.name)
        if lv.call == "window":
            continue  # (below, on one plan)
        if lv.call == "host":
            p = plan(lv, r["path"])
            flat = _source(r, lv, img)
            hs = np.zeros(flat.nbytes + 48, np.uint8)
            o = (-hs.ctypes.data) % 16 + lv.soff
            hs[o:o + flat.nbytes] = flat.view(np.uint8)
            d = _Dst(r, lv, host=True)
            rc, tags, msg = call(p, hs.ctypes.data + o, d.ptr(), 0, nh,
                                 abi.MEM_HOST)
            if rc != 0:
                problems.append("%s: rc %d %r" % (what, rc, msg))
            else:
                d.check(r, want, [(0, nh)], what, problems, log)
            continue
        bands = A.bands(r, lv.g) if lv.call == "bands" else [(0, nh)]
        p = plan(lv, r["path"])
        tells0 = A.tells(r, lv)
        if p is None:
            log.append("%s: set_path refused" % what)
            if "refused" not in tells0:
                problems.append("%s: the forced path refuses the geometry"
                                % what)
        d = _Dst(r, lv)
        stored, again = [], []
        for a, b in bands:
            tells = A.tells(r, lv, lv.doff + a * d.row_b)
            bw = "%s [%d, %d)" % (what, a, b) if lv.call == "bands" else what
            if p is None:
                again.append((a, b))
                continue
            rc, tags, msg = call(p, source(lv), d.ptr(a), a, b)
            log.append("%s: rc %d, %r; the table says %r" % (
                bw, rc, sorted(tags), sorted(tells) or "fast"))
            if rc == abi.EUNSUPPORTED:
                again.append((a, b))
                if "refused" not in tells:
                    problems.append("%s: refused on the fast road (%s)"
                                    % (bw, msg.decode()))
                if r["kernel"] and _ran(r, tags):
                    problems.append("%s: refused, yet %s ran" % (
                        bw, r["kernel"]))
                continue
            if rc != 0:
                problems.append("%s: rc %d %r" % (bw, rc, msg))
                continue
            stored.append((a, b))
            if lv.name == "aligned":
                base = _stages(tags)
                if base & uses:
                    problems.append("%s: the aligned call already shows %r"
                                    % (bw, sorted(base & uses)))
                if r["base"] is not None and base != r["base"]:
                    problems.append("%s: the aligned call shows the stages "
                                    "%r, the row says %r" % (
                                        bw, sorted(base), sorted(r["base"])))
            if "refused" in tells:
                problems.append("%s: the table places it aside (refused), "
                                "the forced path ran it: %r" % (
                                    bw, sorted(tags)))
            else:
                _road(r, tags, base or set(), tells, bw, problems)
        d.check(r, want, stored, what, problems, log)
        if again:
            # what the forced path refused, the automatic path serves: the
            # same pointers (the refused calls left the sentinel there)
            p0 = plan(lv, 0)
            if p0 is None:
                problems.append("%s: the automatic path refuses the plan"
                                % what)
                continue
            served = []
            for a, b in again:
                rc, tags, msg = call(p0, source(lv), d.ptr(a), a, b)
                log.append("%s [%d, %d) automatic path: rc %d, %r" % (
                    what, a, b, rc, sorted(tags)))
                if rc != 0:
                    problems.append("%s [%d, %d): the automatic path: rc %d %r"
                                    % (what, a, b, rc, msg))
                else:
                    served.append((a, b))
            d.check(r, want, stored + served, what + " automatic path",
                    problems, log)
        del d

    wl = [lv for lv in A.levels(r) if lv.call == "window"]
    if wl:
        img, want = wants[0]
        nh = want.shape[0]
        p = plan(wl[0], r["path"])
        sw, sh = img.shape[1], img.shape[0]
        rowe = sw * r["ch"]
        _, r0, r1 = W.bands(nh)[1]
        fa, fb = C.c_int(), C.c_int()
        abi.check(lib.avirhip_band_source_rows(p, r0, r1, C.byref(fa),
                                               C.byref(fb)), "source rows")
        n = fb.value - fa.value + 1
        rows = np.ascontiguousarray(img.reshape(sh, rowe)[fa.value:
                                                          fa.value + n])
        # (the plan's own first-call allocations: one aligned whole frame)
        d = _Dst(r, wl[0])
        call(p, source(wl[0]._replace(soff=0)), d.ptr(), 0, nh)
        staged = False
        for lv in wl:
            what = "%s %s" % (r["name"], lv.name)
            t = _dev(rows, off=lv.soff)
            d = _Dst(r, lv)
            before = lib.avirhip_plan_device_bytes(p)
            capfd.readouterr()
            rc = lib.avirhip_resize_window(
                p, C.c_void_p(t.data_ptr() + lv.soff), abi.MEM_DEVICE,
                fa.value, n, C.c_void_p(d.ptr(r0)), abi.MEM_DEVICE, r0, r1,
                None)
            msg = lib.avirhip_last_error()
            torch.cuda.synchronize()
            tags = _tags(capfd.readouterr().err)
            grow = lib.avirhip_plan_device_bytes(p) - before
            held = lib.avirhip_plan_device_bytes(p)
            fast = A.on_fast_road(r, lv)["window"]
            log.append("%s: rc %d, %r, the plan grew by %d bytes to %d (the "
                       "window has %d); the table says %s" % (
                           what, rc, sorted(tags), grow, held, rows.nbytes,
                           "where it lies" if fast else "staged"))
            if rc != 0:
                problems.append("%s: rc %d %r" % (what, rc, msg))
                continue
            d.check(r, want, [(r0, r1)], what, problems, log)
            if not _ran(r, tags):
                problems.append("%s: no %s line" % (what, r["kernel"]))
            if fast and grow >= rows.nbytes:
                problems.append("%s: a window the kernel takes where it lies "
                                "was staged (%d bytes)" % (what, grow))
            # (the staging frame is made once and kept: the first staged
            # window shows as held bytes, the later ones as no growth at all)
            if not fast:
                if grow < rows.nbytes and not staged:
                    problems.append("%s: the table places it aside (staged), "
                                    "the plan grew by %d bytes" % (what, grow))
                staged = True
    return problems, log


@pytest.mark.parametrize("name", A.NAMES)
def test_alignment(name, capfd):
    r = A.row(name)
    with G.environment(dict(r["env"], AVIRHIP_VERBOSE="1")):
        problems, log = _run_row(r, capfd)
    capfd.readouterr()
    print("\n".join(log))
    assert not problems, "\n".join(problems)
