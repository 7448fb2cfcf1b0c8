"""Every kernel family with the output grid placed off the source frame: the
cases of tests/placement_cases.py (whole-pixel shifts past either edge, grids
larger than the frame, small interior crops, bands that read nothing but a
replicated edge row, whole ratios at half-pixel phases).

Per case: the whole frame on the forced path from a host and from a device
source, the same plan on the generic kernels, row bands into sentinel-filled
destinations, and avirhip_resize_window for the first and the last fifth from
exactly the rows band_source_rows names while the plan's staging holds poison.
Whether the forced path takes the plan is asserted against
placement_cases.expect(); a refused case still runs on the automatic path.

Expected pixels are the reference's (tests/helpers.py), one whole frame per
case. Raw words are compared, the bar is 0 differing elements."""
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import placement_cases as P
from tests import test_gpu_window as TW
from tests import window_cases as W

pytestmark = pytest.mark.gpu

# case id -> the path that executed it (None: refused); filled by the
# parametrised test, read by the test behind it
RAN = {}


def _new_plan(w, obj, arg):
    fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex = w
    ti, to = avir_amd._NP2T[np.dtype(tin)], avir_amd._NP2T[np.dtype(tout)]
    if fe == "lancir":
        return obj.plan(sw, sh, nw, nh, ch, arg, ti, to)
    return obj.plan(sw, sh, nw, nh, ch, float(ex["k"]), arg, ti, to,
                    W.pitch(w) if ex.get("pad") else 0)


@pytest.mark.parametrize("case", P.CASES, ids=P.IDS)
def test_placed_grid(case):
    import torch
    row, w, placed = case
    fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex = w
    lib = abi.load()
    abi.check(lib.avirhip_init(0), "init")
    img = TW._image(w)
    want = TW._want(w, img)
    assert want.shape == (nh, nw, ch) and want.dtype == np.dtype(tout)
    obj, arg = W.front_end(w)
    p = _new_plan(w, obj, arg)
    with P.Desc(case) as d:
        why = P.expect(case, d)
        band_list = P.bands(case, d)
    pitch = W.pitch(w)
    esz, osz = np.dtype(tin).itemsize, np.dtype(tout).itemsize
    rowb = nw * ch * osz
    pfill = np.nan if img.dtype.kind == "f" else np.iinfo(img.dtype).max
    frame = TW._flat(img, pitch, pfill)
    d_frame = TW._dev(frame)
    d_poison = TW._dev(TW._flat(TW._poison(img), pitch, pfill))
    d_scratch = TW._dev_sentinel(nh * rowb)
    problems = []

    def check(what, got_bytes, r0, r1):
        nd = TW._differ(got_bytes, want[r0:r1])
        print("%s: rows [%d, %d): %d of %d elements differ"
              % (what, r0, r1, nd, (r1 - r0) * nw * ch))
        if nd:
            problems.append("%s: %d elements differ" % (what, nd))

    def whole(what):
        got = np.zeros((nh, nw, ch), tout)
        abi.check(lib.avirhip_resize(p, frame.ctypes.data, abi.MEM_HOST,
                                     got.ctypes.data, abi.MEM_HOST, None),
                  what + " host source")
        check(what + " host source", got.view(np.uint8).reshape(-1), 0, nh)
        dst = TW._dev_sentinel(nh * rowb)
        abi.check(lib.avirhip_resize(p, d_frame.data_ptr(), abi.MEM_DEVICE,
                                     dst.data_ptr(), abi.MEM_DEVICE, None),
                  what + " device source")
        torch.cuda.synchronize()
        check(what + " device source", dst.cpu().numpy(), 0, nh)

    # ---- acceptance / refusal against the table
    rc = lib.avirhip_plan_set_path(p, path)
    if rc != 0:
        msg = (lib.avirhip_last_error() or b"").decode()
        assert rc == abi.EUNSUPPORTED and "cannot run this plan" in msg, (rc,
                                                                          msg)
        RAN[P.case_id(case)] = None
        print("path %d refused (%s)" % (path, why))
        assert why is not None, "path %d refused the plan, the table says " \
            "it runs" % path
        # the automatic path serves the call
        abi.check(lib.avirhip_plan_set_path(p, 0), "set_path 0")
        whole("automatic path %d" % lib.avirhip_plan_get_path(p))
        assert not problems, "\n".join(problems)
        return
    assert why is None, "path %d took the plan, the table says refused: %s" \
        % (path, why)
    abi.check(lib.avirhip_plan_set_variant(p, variant), "set_variant")
    took = lib.avirhip_plan_get_path(p)
    assert took == path or path == 0, (took, path)
    RAN[P.case_id(case)] = took
    whole("path %d" % took)

    # ---- row bands into sentinel-filled destinations; the first and the last
    # fifth also from their source window alone
    def poison():
        abi.check(lib.avirhip_resize_window(
            p, d_poison.data_ptr(), abi.MEM_DEVICE, 0, sh,
            d_scratch.data_ptr(), abi.MEM_DEVICE, 0, nh, None), "poison call")

    for name, r0, r1 in band_list:
        G = 2 * rowb  # (guard rows either side of the band)
        dst = TW._dev_sentinel(2 * G + (r1 - r0) * rowb)
        abi.check(lib.avirhip_resize_band(
            p, d_frame.data_ptr(), abi.MEM_DEVICE, dst.data_ptr() + G,
            abi.MEM_DEVICE, r0, r1, None), "band " + name)
        torch.cuda.synchronize()
        out = dst.cpu().numpy()
        check("band " + name, out[G:len(out) - G], r0, r1)
        if not ((out[:G] == TW.SENTINEL).all() and
                (out[len(out) - G:] == TW.SENTINEL).all()):
            problems.append("band %s: bytes outside the band were written"
                            % name)
        a, b = TW._rows_of(lib, p, r0, r1)
        assert (a, b) == W.host_source_rows(w, obj, arg, r0, r1), name
        assert 0 <= a <= b < sh, (name, a, b)
        if name not in ("first", "last"):
            continue
        rows = np.ascontiguousarray(
            frame[a * pitch:b * pitch + sw * ch])
        assert rows.nbytes == ((b - a) * pitch + sw * ch) * esz
        d_rows = TW._dev(rows)
        poison()
        dst = TW._dev_sentinel(2 * G + (r1 - r0) * rowb)
        abi.check(lib.avirhip_resize_window(
            p, d_rows.data_ptr(), abi.MEM_DEVICE, a, b - a + 1,
            dst.data_ptr() + G, abi.MEM_DEVICE, r0, r1, None),
            "window " + name)
        torch.cuda.synchronize()
        out = dst.cpu().numpy()
        check("window %s of source rows [%d, %d]" % (name, a, b),
              out[G:len(out) - G], r0, r1)
        if not ((out[:G] == TW.SENTINEL).all() and
                (out[len(out) - G:] == TW.SENTINEL).all()):
            problems.append("window %s: bytes outside the band were written"
                            % name)

    # ---- the same plan on the generic kernels
    if took != abi.PATH_GENERIC:
        abi.check(lib.avirhip_plan_set_path(p, abi.PATH_GENERIC), "set_path 1")
        abi.check(lib.avirhip_plan_set_variant(p, 0), "set_variant 0")
        whole("generic kernels")
    assert not problems, "\n".join(problems)


def test_every_family_ran_placed_cases_on_its_forced_path():
    """Behind the cases above: no line of the family list is covered by
    refusals alone. k_up2 and k_lanc2: the shifted cases are refused, the
    un-shifted explicit-k case runs on path 4."""
    assert sorted(RAN) == sorted(P.IDS), "run the whole file"
    for row in P.ROWS:
        cases = [c for c in P.CASES if c[0] == row]
        ran = [c for c in cases if c[2][0] != "cover" and
               RAN[P.case_id(c)] is not None and
               RAN[P.case_id(c)] == (c[1][9] or RAN[P.case_id(c)])]
        print("%s: %d of %d cases ran on their forced path" % (
            row, len(ran), len(cases)))
        if row not in ("x2", "lanc2"):
            assert len(ran) >= 2, row
            continue
        on4 = [c for c in cases if c[1][9] == 4]
        for c in on4:
            took = RAN[P.case_id(c)]
            if c[2] == ("cover", "cover"):
                assert took == 4, c
            else:
                assert took is None, c
        assert len(on4) >= 2 and any(c[2] == ("cover", "cover") for c in on4)
        # (... and the shifted call came out right elsewhere)
        assert ran, row
