"""Downsizing by a non-integer ratio of 2 or more (path 5) with half / bfloat16
sources: the streaming-accumulation kernels read them where they lie -- the
exact k_sacc< 4 / 5 > by default, k_sacc2< 4 / 5 > first under
AVIRHIP_VARIANT_SACC_OPTIMISTIC (the exact kernels behind the alarm) -- from
65,536 source pixels on; below that floor the pack pass stays in front.

Expected bits and inputs: tests/sacc16_cases.py (the reference on the exactly
widened float32 source, its float32 result narrowed; word for word, NaN equal
to NaN). The calls are made on device-resident torch tensors through
avirhip_resize_band; the helpers are tests/test_gpu_gp16.py's.

Forced path 5 accepts all four narrow sources (w9, w8, w7, w5): the tests
assert it, none of them runs on the automatic path alone."""
import numpy as np
import pytest
from avir_amd import abi
from tests import sacc16_cases as S
from tests import far_row_cases as F
from tests import test_gpu_gp16 as B
from tests.gpass_route_cases import environment

pytestmark = pytest.mark.gpu

T = S.T
P5 = S.P5
NO_IO16 = B.NO_IO16
FORMS = {"exact": 0, "optimistic": S.V_OPT}
_forms = sorted(FORMS)
_ids = ["%s-%s" % pr for pr in S.PAIRS]


def _over(lib, geom, p, variant=0):
    return B._held_over_float(lib, geom, p, P5, variant)


# ---- 1. every pair ------------------------------------------------------------

@pytest.mark.parametrize("form", _forms)
@pytest.mark.parametrize("path", [0, P5], ids=["auto", "path5"])
@pytest.mark.parametrize("tin,tout", S.PAIRS, ids=_ids)
def test_every_pair(tin, tout, path, form):
    """Every source type into both 16-bit results, both 16-bit sources into
    f32, u8 and u16: whole frame, bands, the odd band alone. Same-type pairs at
    1-4 channels, and on the narrowest rows as well."""
    lib = B._lib()
    same = (tin, tout) in S.SAME
    for name in S.PAIR_SHAPES + (S.NARROW if same else []):
        geom = S.geom(name)
        for ch in ([4, 1, 2, 3] if same else [4]):
            r, p = B._plan(geom, tin, tout, path, FORMS[form], ch=ch)
            assert p is not None, (name, path, ch)
            src, want = S.case(geom, tin, tout, ch)
            what = "%s %s->%s x%d path %d %s" % (name, tin, tout, ch, path, form)
            B._frame_and_bands(lib, p, B._dev(src), want, tout, what)


# ---- 2. held memory -------------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_no_float_copies_on_the_plan(t):
    """Same-type RGBA on forced path 5: neither the float copy of the source
    (sw * sh * 16 bytes) nor the float result (nw * nh * 16) -- `mid` and the
    tables, as the float32 plan. Under AVIRHIP_GP_NO_IO16 a fresh plan holds
    both; below the floor the source copy, as before."""
    lib = B._lib()
    for name in S.HELD_SHAPES + ["floor"]:
        geom = S.geom(name)
        sw, sh, nw, nh = geom
        src, want = S.case(geom, t, t)
        dsrc = B._dev(src)
        what = "%s %s" % (name, t)
        r, p = B._plan(geom, t, t, P5)
        assert p is not None
        B._frame(lib, p, dsrc.data_ptr(), want, t, what)
        over = _over(lib, geom, p)
        print("%s: %d bytes over the float plan (source copy %d, result %d)" %
              (what, over, sw * sh * 16, nw * nh * 16))
        if name != "floor":
            assert over < min(sw * sh, nw * nh) * 16, what
        else:
            assert sw * sh * 16 <= over < sw * sh * 16 + nw * nh * 16, what
        with environment(NO_IO16):
            r2, p2 = B._plan(geom, t, t, P5)
            B._frame(lib, p2, dsrc.data_ptr(), want, t, what + " no io16")
            over2 = _over(lib, geom, p2)
        print("%s under AVIRHIP_GP_NO_IO16: %d bytes over" % (what, over2))
        assert over2 >= sw * sh * 16 + nw * nh * 16, what


# ---- 3. the roads agree -----------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_roads_agree(t):
    """The typed exact road, the typed optimistic road, pack pass and output
    stage (AVIRHIP_GP_NO_IO16), the tiles, the per-op kernels (forced path 1):
    the same bytes."""
    lib = B._lib()
    for name in ("acc", "acc_odd"):
        geom = S.geom(name)
        for ch in (4, 3):
            src, want = S.case(geom, t, t, ch)
            dsrc = B._dev(src)
            what = "%s %s x%d" % (name, t, ch)
            r, p = B._plan(geom, t, t, P5, ch=ch)
            assert p is not None
            got = B._frame(lib, p, dsrc.data_ptr(), want, t, what)
            ro, po = B._plan(geom, t, t, P5, S.V_OPT, ch=ch)
            g = B._frame(lib, po, dsrc.data_ptr(), want, t, what + " optimistic")
            assert g.tobytes() == got.tobytes(), what
            with environment(NO_IO16):
                g = B._frame(lib, p, dsrc.data_ptr(), want, t, what + " no io16")
            assert g.tobytes() == got.tobytes(), what
            tiles = 0
            for path in (2, 3, 1):
                r2, p2 = B._plan(geom, t, t, path, ch=ch)
                if p2 is None:
                    assert path != 1
                    continue
                tiles += (path != 1)
                g = B._frame(lib, p2, dsrc.data_ptr(), want, t,
                             "%s path %d" % (what, path))
                assert g.tobytes() == got.tobytes(), (what, path)
            assert tiles >= 1, what


# ---- 4. chunk seams ---------------------------------------------------------------

@pytest.mark.parametrize("form", _forms)
@pytest.mark.parametrize("chunk", S.CHUNKS)
@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_chunk_seams(t, chunk, form):
    lib = B._lib()
    for name in ("acc_odd", "w9"):
        geom = S.geom(name)
        for ch in (3, 4):
            r, p = B._plan(geom, t, t, P5, FORMS[form], ch=ch)
            assert p is not None, name
            src, want = S.case(geom, t, t, ch)
            with environment({"AVIRHIP_SA_CHUNK": str(chunk)}):
                B._frame_and_bands(lib, p, B._dev(src), want, t,
                                   "%s %s x%d chunk %d %s" % (name, t, ch, chunk,
                                                             form))


# ---- 5. special values ----------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_special_values(t):
    """+-0, denormals (half: of the source's own too), +-Inf, NaN and blocks
    whose overshoot leaves the format, on the exact road and on the optimistic
    one -- where the alarm has to bring the exact kernels in: the branch-free
    launches alone (AVIRHIP_SACC_OPT_ONLY) leave another result. A finite
    frame behind it on the same plan gives its own bits: the alarm is lowered
    per call."""
    lib = B._lib()
    src, ref, want = S.special_case(t)
    c = S.special_classes(t, ref, want)
    print(t, c)
    assert c["pos_inf"] > 0 and c["neg_inf"] > 0 and c["denormal"] > 0
    assert 0 < c["nan"] < c["size"] // 10
    size, out = S.SPECIAL
    geom = size + out
    dsrc = B._dev(src)
    r, p = B._plan(geom, t, t, P5)
    assert p is not None
    got = B._frame(lib, p, dsrc.data_ptr(), want, t, "special %s exact" % t)
    assert _over(lib, geom, p) < min(size[0] * size[1], out[0] * out[1]) * 16
    gf, wf = S.as_f32(got, t), S.as_f32(want, t)
    assert np.array_equal(np.isinf(gf), np.isinf(wf))
    assert np.array_equal(np.isnan(gf), np.isnan(wf))

    ro, po = B._plan(geom, t, t, P5, S.V_OPT)
    assert po is not None
    g = B._frame(lib, po, dsrc.data_ptr(), want, t, "special %s optimistic" % t)
    assert g.tobytes() == got.tobytes()
    # the branch-free kernels alone: 0 * Inf, 0 * NaN in the slots of outputs
    # the sample does not belong to
    import torch
    d = torch.zeros(want.nbytes, dtype=torch.uint8, device="cuda:0")
    with environment({"AVIRHIP_SACC_OPT_ONLY": "1"}):
        B._call(lib, po, dsrc.data_ptr(), d.data_ptr(), 0, out[1])
    alone = B._host(d, t, want.shape)
    differ = int((S.words(alone) != S.words(want)).sum())
    print("%s: the branch-free kernels alone differ at %d words" % (t, differ))
    assert differ > 0
    # a finite frame behind it, same plan
    fin = S.finite_of(src, t)
    fref = S.H.checker_avir(S.as_f32(fin, t), out[0], out[1],
                            out_dtype=np.float32, resbits=16)
    fwant = S.from_f32(fref, t)
    assert np.isfinite(fref).all()
    dfin = B._dev(fin)
    B._frame(lib, po, dfin.data_ptr(), fwant, t, "finite %s optimistic" % t)
    with environment({"AVIRHIP_SACC_OPT_ONLY": "1"}):
        B._frame(lib, po, dfin.data_ptr(), fwant, t,
                 "finite %s branch-free alone" % t)
    B._frame(lib, po, dsrc.data_ptr(), want, t, "special %s again" % t)


# ---- 6. refusals and layout -------------------------------------------------------

@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_refusals_and_layout(t):
    """A source base 1 byte off: the pack pass's float copy, rc == 0, the same
    bits. A base 2 or 6 bytes into its allocation, a row pitch of sw * ch + 1 /
    + 5 elements with NaN between the rows: read where they lie. Every source
    is an allocation that ends with the image's last byte."""
    lib = B._lib()
    for name, ch in (("acc", 4), ("acc_odd", 3), ("acc_odd", 4)):
        geom = S.geom(name)
        sw, sh, nw, nh = geom
        src, want = S.case(geom, t, t, ch)
        what = "%s %s x%d" % (name, t, ch)
        both = (sw * sh + nw * nh) * 16
        small = min(sw * sh, nw * nh) * 16

        r, p = B._plan(geom, t, t, P5, ch=ch)
        off = B._dev(src, off=1)
        B._frame(lib, p, off.data_ptr() + 1, want, t, what + " source 1 byte off")
        over = _over(lib, geom, p)
        assert sw * sh * 16 <= over < both, (what, over)

        for o in (2, 6):
            r, p = B._plan(geom, t, t, P5, ch=ch)
            off = B._dev(src, off=o)
            B._frame(lib, p, off.data_ptr() + o, want, t,
                     "%s %d bytes in" % (what, o))
            over = _over(lib, geom, p)
            assert over < small, (what, o, over)

        for extra in (1, 5):
            pitch = sw * ch + extra
            for form in _forms:
                r, p = B._plan(geom, t, t, P5, FORMS[form], pitch=pitch, ch=ch)
                dflat = B._dev(S.padded(src, pitch, t))
                B._frame_and_bands(lib, p, dflat, want, t,
                                   "%s pitch + %d %s" % (what, extra, form))
                over = _over(lib, geom, p, FORMS[form])
                assert over < small, (what, extra, form, over)


# ---- 7. rows far from the base ----------------------------------------------------

# A row of tests/far_row_cases.py's vocabulary: bfloat16 RGBA, `acc`. The pass
# kernels of a plan are dropped when its frame ends 2 GiB or more from its base
# counted in 4-byte elements (gpass.hip:971, the guard of every kernel of the
# path): forced path 5 cannot be given a 16-bit frame whose rows lie more than
# 1 GiB from the base, whatever the loaders' own 64-bit row addresses would
# reach. So: `under`, the farthest rows that guard admits, on the typed road;
# `wrap`, rows beyond 4 GiB, where set_path has to refuse and the automatic
# path has to give the same bits.
FAR = dict(F.row("sacc2_u16c4"))
FAR.update(name="sacc16_bf16c4", tin="bf16", tout="bf16", bits=16, ch=4,
           sw=S.geom("acc")[0], sh=S.geom("acc")[1], nw=S.geom("acc")[2],
           nh=S.geom("acc")[3])


@pytest.mark.parametrize("level", ["under", "wrap"])
def test_rows_far_from_the_base(level):
    import torch
    from tests import test_gpu_far_rows as R
    lib = B._lib()
    lv = F.level(FAR, level)
    if lv.dropped:
        print("sacc16 %s: dropped, %s" % (level, lv.dropped))
        pytest.skip(lv.dropped)
    assert lv.inside == (level == "under")
    geom = S.geom("acc")
    sw, sh, nw, nh = geom
    src, want = S.case(geom, "bf16", "bf16")
    row_b = sw * 4 * 2
    far = (sh - 1) * lv.pitch * 2
    print("sacc16 %s: pitch %d elements, the last row %.2f GiB from the base" %
          (level, lv.pitch, far / 2.0 ** 30))
    # (`wrap`: the image's span exceeds 2^32 -- the last row ends beyond it)
    assert far + row_b > (F.GIB4 if level == "wrap" else
                          (1 << 30) - (8 << 20))
    dsrc = R._Pitched(sh, row_b, lv.pitch * 2)
    dsrc.put(src)
    r, p = B._plan(geom, "bf16", "bf16", P5, pitch=lv.pitch)
    if level == "under":
        assert p is not None
        for form in _forms:
            r, p = B._plan(geom, "bf16", "bf16", P5, FORMS[form], pitch=lv.pitch)
            B._frame(lib, p, dsrc.ptr(), want, "bf16", "far %s %s" % (level, form))
            d = torch.zeros(R.LAST * nw * 8, dtype=torch.uint8, device="cuda:0")
            B._call(lib, p, dsrc.ptr(), d.data_ptr(), nh - R.LAST, nh)
            S.same(B._host(d, "bf16", want[nh - R.LAST:].shape),
                   want[nh - R.LAST:], "bf16", "far %s %s last rows" % (level,
                                                                        form))
            assert _over(lib, geom, p, FORMS[form]) < nw * nh * 16
    else:
        assert p is None, "the guard of gpass.hip:971 admitted the frame"
        r, p = B._plan(geom, "bf16", "bf16", 0, pitch=lv.pitch)
        assert p is not None
        B._frame(lib, p, dsrc.ptr(), want, "bf16", "far %s auto" % level)
    del dsrc
    torch.cuda.empty_cache()


# ---- 8. the automatic path ----------------------------------------------------

def _auto_path(lib, geom, t, ch=4):
    r, p = B._plan(geom, t, t, 0, ch=ch)
    return lib.avirhip_plan_get_path(p)


@pytest.mark.parametrize("t", ["f16", "bf16"])
def test_automatic_path(t):
    """From S.AUTO_MINPIX source pixels on, a 16-bit source with both axes on
    the accumulation kernels takes path 5 by itself; below it, and below the
    floor, the path it took before (that of a plan made under
    AVIRHIP_GP_NO_IO16, which knows no typed road)."""
    lib = B._lib()
    for geom, ch in S.AUTO_P5:
        assert geom[0] * geom[1] >= S.AUTO_MINPIX
        assert _auto_path(lib, geom, t, ch) == P5, (geom, ch)
        with environment(NO_IO16):
            before = _auto_path(lib, geom, t, ch)
        print("%r x%d %s: path 5, before: path %d" % (geom, ch, t, before))
        assert before != P5
    assert S.geom("floor") in S.AUTO_BEFORE and S.geom("acc") in S.AUTO_BEFORE
    for geom in S.AUTO_BEFORE:
        assert geom[0] * geom[1] < S.AUTO_MINPIX
        now = _auto_path(lib, geom, t)
        with environment(NO_IO16):
            before = _auto_path(lib, geom, t)
        assert now == before and now != P5, (geom, now, before)
    # one frame at the crossing: the reference's bits on the path it now takes
    geom, ch = S.AUTO_P5[0]
    src, want = S.case(geom, t, t, ch)
    r, p = B._plan(geom, t, t, 0, ch=ch)
    dsrc = B._dev(src)
    B._frame(lib, p, dsrc.data_ptr(), want, t, "auto %r %s" % (geom, t))
    assert _over(lib, geom, p) < min(geom[0] * geom[1], geom[2] * geom[3]) * 16
