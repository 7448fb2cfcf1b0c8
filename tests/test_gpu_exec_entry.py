"""The execute entry (avir_amd/csrc/api.cpp: exec_any, src_route) walked by
the rows of its source-route table -- where the kernels of a call read the
source from, and which bytes move before they do:

  1 device frame, no bytes shared with dst   read where it lies
  2 device frame sharing bytes with dst      whole frame copied aside, D2D
  3 host frame                               whole frame uploaded
  4 window, marching kernel, device, apart   read where it lies (virtual base)
  5 window, marching kernel, host or shared  window-sized staging buffer
  6 window, any other plan                   window to its place in a frame

Every row runs once to a device and once to a host destination. (A host
destination shares no bytes with a device frame: row 2's host run is the
in-place HOST call, source and destination the same bytes.) Two plans of
tests/window_cases.py: its smallest exact-2x float RGBA case (rows 4 and 5)
and its smallest integer case that is not 2x (the others).

Before each call an all-poison whole-frame host call fills the plan's staging
buffers, and a window lies between poison rows. Expected pixels are the
reference's (tests/helpers.py), one frame per source image; raw words are
compared, the bar is 0 differing elements.

The last test orders calls on one scratch-using plan across two non-default
streams (api.cpp: order_behind_last_call)."""
import functools
import numpy as np
import pytest
from avir_amd import abi
from tests import test_gpu_window as TW
from tests import window_cases as W

pytestmark = pytest.mark.gpu


def _is_2x(c):
    return c[3] == 2 * c[1] and c[4] == 2 * c[2]


def _smallest(pred):
    return min((c for c in W.CASES if pred(c)),
               key=lambda c: c[1] * c[2] + c[3] * c[4])


PLANS = {
    "up2": _smallest(lambda c: _is_2x(c) and c[5] == 4 and c[11].get("native")
                     and c[6] == c[7] == W.F32 and not c[11].get("pad")),
    "other": _smallest(lambda c: not _is_2x(c) and not c[11].get("pad")
                       and np.dtype(c[6]).kind == "u"),
}


@functools.lru_cache(maxsize=None)
def _ref(key, seed):
    """(source image, the reference's frame), computed once and shared:
    nothing here writes to either."""
    img = TW._image(PLANS[key], seed)
    want = TW._want(PLANS[key], img)
    want.setflags(write=False)
    return img, want


class _Setup:
    """One plan of PLANS, its images and the calls of this file."""

    def __init__(self, key, seed=0):
        c = PLANS[key]
        self.sw, self.sh, self.nw, self.nh, self.ch = c[1:6]
        self.lib = abi.load()
        abi.check(self.lib.avirhip_init(0), "init")
        self.img, self.want = _ref(key, seed)
        assert self.want.shape == (self.nh, self.nw, self.ch)
        self.obj, arg = W.front_end(c)
        self.p = TW._plan(c, self.obj, arg)
        self.bad = TW._poison(self.img)
        self.rowb = self.sw * self.ch * self.img.dtype.itemsize
        self.orowb = self.nw * self.ch * self.want.dtype.itemsize
        f = self.nh // 5
        self.r0, self.r1 = 2 * f, 3 * f  # the window rows' band
        self.a, self.b = TW._rows_of(self.lib, self.p, self.r0, self.r1)
        assert 0 < self.a <= self.b < self.sh - 1

    def poison(self):
        """An all-poison whole-frame host call: the plan's source staging
        buffer holds poison, its destination staging buffer what came of it."""
        junk = np.empty(self.nh * self.orowb, np.uint8)
        abi.check(self.lib.avirhip_resize(
            self.p, self.bad.ctypes.data, abi.MEM_HOST, junk.ctypes.data,
            abi.MEM_HOST, None), "poison call")

    def window(self):
        """The frame with every row outside [a, b] poison."""
        buf = self.bad.copy()
        buf[self.a:self.b + 1] = self.img[self.a:self.b + 1]
        return buf

    def call(self, src, mem, host_dst, win=False, dst=None, stream=None):
        """One call -> the differing elements of its rows. `src`: the frame's
        first byte; `win`: the call is a window call for rows [r0, r1) that
        is handed rows [a, b]; `dst`: a device address to store at."""
        import torch
        r0, r1 = (self.r0, self.r1) if win else (0, self.nh)
        nbytes = (r1 - r0) * self.orowb
        if host_dst:
            out = np.full(nbytes, TW.SENTINEL, np.uint8)
            to, tomem = out.ctypes.data, abi.MEM_HOST
        elif dst is None:
            d = TW._dev_sentinel(nbytes)
            to, tomem = d.data_ptr(), abi.MEM_DEVICE
        else:
            to, tomem = dst, abi.MEM_DEVICE
        self.poison()
        if win:
            rc = self.lib.avirhip_resize_window(
                self.p, src + self.a * self.rowb, mem, self.a,
                self.b - self.a + 1, to, tomem, r0, r1, stream)
        else:
            rc = self.lib.avirhip_resize(self.p, src, mem, to, tomem, stream)
        abi.check(rc, "call")
        torch.cuda.synchronize()
        if dst is not None:
            return None
        got = out if host_dst else d.cpu().numpy()
        return TW._differ(got, self.want[r0:r1])


HOST_DST = pytest.mark.parametrize("host_dst", [False, True],
                                   ids=["device-dst", "host-dst"])


@HOST_DST
def test_device_frame_apart_from_dst(host_dst):
    S = _Setup("other")
    d_img = TW._dev(S.img)
    assert S.call(d_img.data_ptr(), abi.MEM_DEVICE, host_dst) == 0


@HOST_DST
def test_frame_sharing_bytes_with_dst(host_dst):
    """In place: the result (not larger) at the source's first byte."""
    import torch
    S = _Setup("other")
    nbytes = S.nh * S.orowb
    assert nbytes <= S.img.nbytes
    if host_dst:
        buf = S.img.copy()
        S.poison()
        abi.check(S.lib.avirhip_resize(
            S.p, buf.ctypes.data, abi.MEM_HOST, buf.ctypes.data, abi.MEM_HOST,
            None), "in-place host call")
        torch.cuda.synchronize()
        got = buf.view(np.uint8).reshape(-1)[:nbytes]
    else:
        d_buf = TW._dev(S.img)
        S.call(d_buf.data_ptr(), abi.MEM_DEVICE, False, dst=d_buf.data_ptr())
        got = d_buf[:nbytes].cpu().numpy()
    assert TW._differ(got, S.want) == 0


@HOST_DST
def test_host_frame(host_dst):
    S = _Setup("other")
    assert S.call(S.img.ctypes.data, abi.MEM_HOST, host_dst) == 0


@HOST_DST
def test_device_window_on_the_marching_kernel(host_dst):
    S = _Setup("up2")
    assert S.lib.avirhip_plan_get_path(S.p) == abi.PATH_UP2
    d_win = TW._dev(S.window())
    assert S.call(d_win.data_ptr(), abi.MEM_DEVICE, host_dst, win=True) == 0


@HOST_DST
def test_window_copied_aside_for_the_marching_kernel(host_dst):
    """A host window; and, to a device destination, a device window whose
    first byte is also the band's."""
    S = _Setup("up2")
    win = S.window()
    assert S.call(win.ctypes.data, abi.MEM_HOST, host_dst, win=True) == 0
    if not host_dst:
        nbytes = (S.r1 - S.r0) * S.orowb
        rows = np.ascontiguousarray(S.img[S.a:S.b + 1]).reshape(-1)
        both = np.full(max(rows.nbytes, nbytes) // 4 + 64, np.nan, np.float32)
        both[:rows.size] = rows
        d_both = TW._dev(both)
        S.call(d_both.data_ptr() - S.a * S.rowb, abi.MEM_DEVICE, False,
               win=True, dst=d_both.data_ptr())
        got = d_both[:nbytes].cpu().numpy()
        assert TW._differ(got, S.want[S.r0:S.r1]) == 0


@HOST_DST
def test_window_staged_in_a_frame(host_dst, monkeypatch):
    """Device and host windows of a plan without a marching kernel; a device
    window of the marching kernel's plan with AVIRHIP_NO_NATIVE_WINDOW set."""
    S = _Setup("other")
    win = S.window()
    d_win = TW._dev(win)
    assert S.call(d_win.data_ptr(), abi.MEM_DEVICE, host_dst, win=True) == 0
    assert S.call(win.ctypes.data, abi.MEM_HOST, host_dst, win=True) == 0
    S = _Setup("up2")
    d_win = TW._dev(S.window())
    monkeypatch.setenv("AVIRHIP_NO_NATIVE_WINDOW", "1")
    assert S.call(d_win.data_ptr(), abi.MEM_DEVICE, host_dst, win=True) == 0


def test_calls_that_change_the_stream():
    """Two calls on two non-default streams back to back on one plan whose
    kernels use its scratch buffers, then a third on the first stream: each
    has to wait for what the one before it still holds. The second call's
    source is another image, so a call that ran into its neighbour's scratch
    shows wrong pixels."""
    import torch
    S = _Setup("other")
    img2, want2 = _ref("other", 1)
    s1, s2 = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    d_img, d_img2 = TW._dev(S.img), TW._dev(img2)
    jobs = [(d_img, s1, S.want), (d_img2, s2, want2), (d_img, s1, S.want)]
    dsts = [TW._dev_sentinel(S.nh * S.orowb) for _ in jobs]
    S.poison()
    torch.cuda.synchronize()
    for (src, s, _), d in zip(jobs, dsts):
        abi.check(S.lib.avirhip_resize(
            S.p, src.data_ptr(), abi.MEM_DEVICE, d.data_ptr(), abi.MEM_DEVICE,
            s.cuda_stream), "call on a stream")
    torch.cuda.synchronize()
    nd = [TW._differ(d.cpu().numpy(), want) for (_, _, want), d in zip(jobs, dsts)]
    print("differing elements of the three calls: %r" % (nd,))
    assert nd == [0, 0, 0]
