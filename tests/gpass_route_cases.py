"""The route table of tests/test_gpu_gpass_routes.py and
tools/gpass_route_trace.py: one row per outcome of gpass_route
(avir_amd/csrc/gpass.hip: route_lancir, route_avir), the calls that walk it,
and the kernels a trace of the row has to show (profiles/gpass_route/).

A call is a case of tests/window_cases.py -- (front end, sw, sh, nw, nh, ch,
tin, tout, resbits, path, variant, extras) -- on a plan forced to PATH_GPASS,
with the environment it runs under and the source images it resizes in turn
("clean", or "dirty": an Inf and a NaN planted). Shapes are those of the
path-5 tests of tests/test_gpu_parity.py, the smallest that take the row."""
import ctypes as C
import os
import numpy as np
import avir_amd
from avir_amd import abi
from tests import refbind as rb
from tests import window_cases as W

U8, F32 = np.uint8, np.float32
P5 = abi.PATH_GPASS
V_UPG2, V_UPGF = abi.VARIANT_UPG_TWO_PASS, abi.VARIANT_UPG_FUSED
V_OPT, V_LADDER = abi.VARIANT_SACC_OPTIMISTIC, abi.VARIANT_SACC_LADDER
CLEAN = ("clean",)
ALARM = ("clean", "dirty", "clean")
MIN13 = {"AVIRHIP_GH2_MIN_NT": "13"}


def _c(fe, sw, sh, nw, nh, ch, tin, tout, variant=0, env=None, images=CLEAN,
       **ex):
    bits = 0 if fe == "lancir" else (8 if tout == U8 else 16)
    return ((fe, sw, sh, nw, nh, ch, tin, tout, bits, P5, variant, ex),
            env or {}, images)


# (row, calls, kernel name prefixes in launch order per call and image:
# what `tools/gpass_route_trace.py --check` holds a trace against)
ROWS = [
    ("avir_fused",
     [_c("avir", 64, 48, 100, 77, 4, F32, F32, V_UPGF),
      _c("avir", 64, 48, 100, 77, 4, F32, U8, V_UPGF)],
     [["k_gf"], ["k_gf"]]),
    ("avir_two_pass_gather",
     [_c("avir", 64, 48, 100, 77, 4, F32, F32, V_UPG2),
      _c("avir", 64, 48, 100, 77, 4, F32, U8, V_UPG2)],
     [["k_gh", "k_gv"], ["k_gh", "k_gv"]]),
    ("avir_two_pass_raw_gather",
     [_c("avir", 64, 48, 100, 77, 3, U8, U8)],
     [["k_gh", "k_gv"]]),
    ("avir_acc_exact",
     [_c("avir", 300, 200, 100, 67, 4, F32, F32)],
     [["k_sacc<", "k_sacc<"]]),
    ("avir_optimistic",
     [_c("avir", 300, 200, 100, 67, 4, F32, F32, V_OPT, images=ALARM),
      _c("avir", 300, 200, 100, 67, 3, F32, F32, images=ALARM)],
     [["k_sacc2v", "k_sacc2v", "k_sacc<", "k_sacc<"]] * 2),
    ("avir_acc_finite",
     [_c("avir", 300, 200, 100, 67, 3, U8, U8),
      _c("avir", 300, 200, 100, 67, 3, U8, U8, V_LADDER)],
     [["k_sacc2<", "k_sacc2v"], ["k_sacc<", "k_sacc<"]]),
    ("avir_between_1_and_2",
     [_c("avir", 520, 300, 346, 206, 4, F32, F32),
      _c("avir", 927, 421, 482, 226, 4, F32, F32),
      _c("avir", 520, 300, 346, 206, 4, F32, F32, env=MIN13),
      _c("avir", 927, 421, 482, 226, 4, F32, F32, env=MIN13)],
     [["k_gh<", "k_gv"], ["k_gh2", "k_gv"], ["k_gh2", "k_gv"],
      ["k_gh2", "k_gv"]]),
    # (257x260 -> 64x129 does not take path 5: 257 -> 64 is k > 4, a halving
    # FIR in front of the chain. 90x300 -> 200x120, from the same list of
    # test_avir_pass_kernels_store_integer_images_themselves: upsizing by 2.2
    # horizontally, k = 2.5 vertically)
    ("avir_mixed_axes",
     [_c("avir", 90, 300, 200, 120, 3, U8, U8)],
     [["k_gh", "k_sacc"]]),
    ("lancir_fused",
     [_c("lancir", 64, 48, 100, 77, 4, F32, F32)],
     [["k_lf"]]),
    # (61x45 RGB uint8 has rows of 183 bytes: the raw promise fails and the
    # pack pass runs. 128x96 -> 333x250, the smallest shape of the same list of
    # test_lancir_fused_upsizing_kernel_reads_raw_images with a dword pitch, at
    # a ratio where the fusion still pays for a uint8 result)
    ("lancir_fused_owner",
     [_c("lancir", 128, 96, 333, 250, 3, U8, U8)],
     [["k_lf"]]),
    ("lancir_two_pass",
     [_c("lancir", 64, 48, 100, 77, 4, F32, F32, V_UPG2),
      _c("lancir", 61, 45, 100, 77, 3, U8, U8, V_UPG2),
      _c("lancir", 300, 200, 100, 67, 4, F32, F32)],
     [["k_gv", "k_gh"], ["k_pack", "k_gv", "k_gh"], ["k_gv", "k_gh"]]),
    # (an odd source pitch: the raw promise fails, the pack pass runs)
    ("lancir_odd_pitch",
     [_c("lancir", 100, 60, 170, 141, 3, U8, U8, pad=1)],
     [["k_pack", "k_lf"]]),
]

NAMES = [r[0] for r in ROWS]
# (the refusal row of the test file launches on the automatic path only: it is
# not traced)


def row(name):
    return ROWS[NAMES.index(name)]


def image(c, kind):
    """The source of a call, (sh, sw, ch); "dirty": an Inf and a NaN inside."""
    fe, sw, sh, nw, nh, ch, tin = c[:7]
    if np.dtype(tin).kind == "u":
        return rb.lcg_u8((sh, sw, ch, 1), seed=sw + ch).reshape(sh, sw, ch)
    a = rb.lcg_f32((sh, sw, ch), seed=7 * sw + ch)
    if kind == "dirty":
        a = a.copy()
        a[sh // 3, sw // 2, 0] = np.inf
        a[2 * sh // 3, sw // 4, ch - 1] = np.nan
    return a


def flat(img, pitch):
    """(rows, sw, ch) -> the rows `pitch` elements apart, the last one ending
    with its pixels."""
    rows, sw, ch = img.shape
    out = np.zeros(rows * pitch, img.dtype)
    out.reshape(rows, pitch)[:, :sw * ch] = img.reshape(rows, sw * ch)
    return np.ascontiguousarray(out[:(rows - 1) * pitch + sw * ch])


def bands(nh):
    return [(0, nh // 3), (nh // 3, nh // 3 + 1), (nh // 3 + 1, nh)]


def plan(c, lib=None, path=P5):
    """-> (front-end object: keeps the plan alive, plan) on `path`."""
    fe, sw, sh, nw, nh, ch, tin, tout, bits, _, variant, ex = c
    lib = lib or abi.load()
    obj, arg = W.front_end(c)
    ti, to = avir_amd._NP2T[np.dtype(tin)], avir_amd._NP2T[np.dtype(tout)]
    if fe == "lancir":
        p = obj.plan(sw, sh, nw, nh, ch, arg, ti, to)
    else:
        p = obj.plan(sw, sh, nw, nh, ch, 0.0, arg, ti, to, 0)
    abi.check(lib.avirhip_plan_set_path(p, path), "set_path %d" % path)
    abi.check(lib.avirhip_plan_set_variant(p, variant), "set_variant")
    if path:
        assert lib.avirhip_plan_get_path(p) == path
    return obj, p


class environment(object):
    """`with environment(env):` -- the variables of a call, put back after."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.keep = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def run_device(lib, p, c, dsrc, row_bands, dst_off=0):
    """Output rows `row_bands` of device source `dsrc` (a torch uint8 tensor)
    into a zeroed device image that starts `dst_off` bytes into its
    allocation -> (return codes, the image as a numpy array)."""
    import torch
    fe, sw, sh, nw, nh, ch, tin, tout = c[:8]
    rowb = nw * ch * np.dtype(tout).itemsize
    ddst = torch.zeros(nh * rowb + dst_off + 64, dtype=torch.uint8,
                       device="cuda:0")
    rcs = [lib.avirhip_resize_band(
        p, C.c_void_p(dsrc.data_ptr()), abi.MEM_DEVICE,
        C.c_void_p(ddst.data_ptr() + dst_off + a * rowb), abi.MEM_DEVICE, a, b,
        None) for (a, b) in row_bands]
    torch.cuda.synchronize()
    got = ddst[dst_off:dst_off + nh * rowb].cpu().numpy().view(tout)
    return rcs, got.reshape(nh, nw, ch)


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)
                            ).to("cuda:0")
