"""Every marching kernel at forced chunk lengths and at every seam
(tests/chunk_cases.py: one row per kernel family), against the reference bit
for bit.

A row's sums never depend on where a chunk starts, so every chunk length must
give the same bits:

  forced chunks   the whole frame under every length of the row's stages, each
                  knob on its own and, in the two-pass families, both together;
                  the length in force, the strips and the work items are read
                  back from the library's AVIRHIP_VERBOSE line, so a knob that
                  did nothing fails
  band boundaries every output row r cuts the frame into [0, r) and [r, nh):
                  a band's chunk grid starts at its own first row, so this
                  moves every seam over every row (k_lanc2 / k_lanc2h chunk on
                  the frame's grid: they are walked at cq 2, 10 and 26)
  windows         avirhip_resize_window around three seams, the source holding
                  only the rows avirhip_band_source_rows names, between NaN /
                  complement rows

Expected pixels are the reference's (tests/helpers.py), one frame per
geometry, never written to; raw words are compared, the bar is 0. No special
values are planted, so no NaN arises on either side."""
import ctypes as C
import os
import re
import numpy as np
import pytest
import avir_amd
from avir_amd import abi
from tests import helpers as H
from tests import refbind as rb
from tests import chunk_cases as CC
from tests import dnf16_cases as D16

pytestmark = pytest.mark.gpu

T = dict(D16.T, f64=(abi.F64, np.float64))
ENV_NAMES = ("AVIRHIP_VERBOSE", "AVIRHIP_LANC2_CQ", "AVIRHIP_DNF_CROWS",
             "AVIRHIP_GH_CHUNK", "AVIRHIP_GV_CHUNK", "AVIRHIP_GF_CHUNK",
             "AVIRHIP_LF_CHUNK", "AVIRHIP_SA_CHUNK", "AVIRHIP_SA_CHUNK_V",
             "AVIRHIP_GH2_MIN_NT", "AVIRHIP_UP64_RH", "AVIRHIP_UP64_EPL",
             "AVIRHIP_UP64_HB", "AVIRHIP_UP64_VW")
LINE = re.compile(r"^(k_\w+): (\d+) items \(strips (\d+), (\w+) (-?\d+)"
                  r"((?:, \w+ \w+)*)\)", re.M)


@pytest.fixture(scope="module", autouse=True)
def _device():
    lib = abi.load()
    assert lib.avirhip_device_count() >= 1, "no gfx950 device"
    abi.check(lib.avirhip_init(0), "init")


@pytest.fixture()
def knob():
    """sets the chunk knobs for one call (the launchers read them per call);
    the environment is put back after the test"""
    saved = {n: os.environ.pop(n, None) for n in ENV_NAMES}

    def put(env):
        for n in ENV_NAMES:
            os.environ.pop(n, None)
        for k, v in env.items():
            assert k in ENV_NAMES, k
            os.environ[k] = str(v)
    yield put
    for n, v in saved.items():
        os.environ.pop(n, None)
        if v is not None:
            os.environ[n] = v


def _lines(err):
    """The launchers' lines of a call: [dict(kernel, items, strips, field,
    length, + the line's further fields)]."""
    out = []
    for m in LINE.finditer(err):
        d = dict(kernel=m.group(1), items=int(m.group(2)),
                 strips=int(m.group(3)), field=m.group(4),
                 length=int(m.group(5)))
        for kv in m.group(6).split(", ")[1:]:
            k, v = kv.split(" ")
            d[k] = v if k == "pass" else int(v)
        out.append(d)
    return out


def _of(lines, st):
    return [x for x in lines if x["kernel"] == st.kernel and
            (st.tag is None or x.get("pass") == st.tag)]


# ---- a row's source, expectation and plan

_CASES = {}


def _case(call):
    """(source, expected image): the reference runs once per call."""
    fe, sw, sh, nw, nh, ch, tin, tout, path, variant, env, ex = call
    key = (fe, sw, sh, nw, nh, ch, tin, tout, ex.get("fp", 1))
    if key in _CASES:
        return _CASES[key]
    seed = 31 * sw + sh + ch
    if tin == "f64":
        # (mantissa bits a float does not hold)
        src = (rb.lcg_f32((sh, sw, ch), seed=seed).astype(np.float64) +
               rb.lcg_f32((sh, sw, ch), seed=seed + 1).astype(np.float64) *
               2.0 ** -25)
    else:
        src = D16.source((sh, sw, ch), tin, seed=seed)
    wide = D16.as_f32(src, tin) if tin in ("f16", "bf16") else src
    rt = np.float32 if tout in ("f16", "bf16") else T[tout][1]
    if fe == "lancir":
        ref = H.checker_lancir(wide, nw, nh, out_dtype=rt)
    else:
        kw = {}
        if ex.get("fp") == abi.FPCLASS_DOUBLE:
            assert H.need_ref("the double class")
            kw["variant"] = 4
        ref = H.checker_avir(wide, nw, nh, out_dtype=rt,
                             resbits=8 if tout == "u8" else 16, threads=8, **kw)
    want = np.ascontiguousarray(D16.from_f32(ref, tout))
    assert want.shape == (nh, nw, ch) and want.dtype == np.dtype(T[tout][1])
    src.setflags(write=False)
    want.setflags(write=False)
    _CASES[key] = (src, want)
    return _CASES[key]


def _plan(call):
    """(front-end object: keeps the plan alive, plan, its path) on the row's
    forced path / variant; a refusal fails."""
    fe, sw, sh, nw, nh, ch, tin, tout, path, variant, env, ex = call
    lib = abi.load()
    if fe == "lancir":
        obj = avir_amd.CLancIR()
        p = obj.plan(sw, sh, nw, nh, ch, None, T[tin][0], T[tout][0])
    else:
        obj = avir_amd.CImageResizer(8 if tout == "u8" else 16,
                                     aFpPack=ex.get("fp", 1))
        p = obj.plan(sw, sh, nw, nh, ch, 0.0, None, T[tin][0], T[tout][0], 0)
    abi.check(lib.avirhip_plan_set_path(p, path), "set_path %d" % path)
    abi.check(lib.avirhip_plan_set_variant(p, variant), "set_variant")
    got = lib.avirhip_plan_get_path(p)
    assert path == 0 or got == path
    return obj, p, got


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)
                            .copy()).to("cuda:0")


def _ok(lib, rc, what):
    """A refused call fails the test; a device fault ends the session: nothing
    more may run on a device that has faulted."""
    if rc != 0:
        msg = (lib.avirhip_last_error() or b"?").decode()
        if "illegal memory access" in msg or "hipError" in msg:
            pytest.exit("%s: rc %d (%s)" % (what, rc, msg), returncode=3)
        raise AssertionError("%s: rc %d (%s)" % (what, rc, msg))


def _band(lib, p, dsrc, ddst, rowb, r0, r1, what):
    _ok(lib, lib.avirhip_resize_band(
        p, dsrc.data_ptr(), abi.MEM_DEVICE, ddst.data_ptr() + r0 * rowb,
        abi.MEM_DEVICE, r0, r1, None), what)


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32,
                   8: np.uint64}[a.dtype.itemsize])


def _differ(got_bytes, want):
    w = _words(want).reshape(-1)
    g = np.ascontiguousarray(got_bytes).view(w.dtype)
    assert g.size == w.size
    bad = np.flatnonzero(g != w)
    if not len(bad):
        return ""
    per_row = want.shape[1] * want.shape[2]
    return "%d of %d raw words differ, first in row %d" % (
        len(bad), w.size, bad[0] // per_row)


class _Frame(object):
    """A row's call on the device: source, plan, a destination image."""

    def __init__(self, call):
        import torch
        self.call = call
        self.src, self.want = _case(call)
        self.obj, self.p, self.path = _plan(call)
        self.lib = abi.load()
        self.dsrc = _dev(self.src)
        self.nh = call[4]
        self.rowb = self.want.nbytes // self.nh
        self.dwant = _dev(self.want)
        self.dpoison = ~self.dwant    # every stale byte differs
        self.ddst = torch.empty_like(self.dwant)

    def whole(self, what):
        """-> "" or what differs from the reference"""
        import torch
        self.ddst.copy_(self.dpoison)
        _band(self.lib, self.p, self.dsrc, self.ddst, self.rowb, 0, self.nh,
              what)
        torch.cuda.synchronize()
        assert self.lib.avirhip_plan_get_path(self.p) == self.path, what
        return _differ(self.ddst.cpu().numpy(), self.want)

    def cut_at_every_row(self, what):
        """Bands [0, r) and [r, nh) for every r -> the rows r that differ."""
        import torch
        bad = []
        for r in range(1, self.nh):
            self.ddst.copy_(self.dpoison)
            for r0, r1 in ((0, r), (r, self.nh)):
                _band(self.lib, self.p, self.dsrc, self.ddst, self.rowb, r0,
                      r1, what)
            torch.cuda.synchronize()
            if not torch.equal(self.ddst, self.dwant):
                bad.append(r)
        assert self.lib.avirhip_plan_get_path(self.p) == self.path, what
        return bad

    def window(self, r0, r1, what):
        """Rows [r0, r1) from a compact device window between poison rows ->
        "" or what differs."""
        import torch
        lib, src = self.lib, self.src
        a, b = C.c_int(), C.c_int()
        abi.check(lib.avirhip_band_source_rows(self.p, r0, r1, C.byref(a),
                                               C.byref(b)), "band_source_rows")
        a, b = a.value, b.value
        assert 0 <= a <= b < src.shape[0], (a, b)
        G = 8
        rows = src[a:b + 1]
        if src.dtype.kind == "f":
            fill = np.full((G,) + src.shape[1:], np.nan, src.dtype)
            big = np.concatenate([fill, rows, fill])
        elif self.call[6] == "bf16":
            fill = np.full((G,) + src.shape[1:], D16.NAN, src.dtype)
            big = np.concatenate([fill, rows, fill])
        else:
            # (the complement of the rows that lie there in the frame)
            up = ~src[np.clip(np.arange(a - G, a), 0, src.shape[0] - 1)]
            dn = ~src[np.clip(np.arange(b + 1, b + 1 + G), 0,
                              src.shape[0] - 1)]
            big = np.concatenate([up, rows, dn])
        dbig = _dev(big)
        off = G * rows[0].nbytes
        n = (r1 - r0) * self.rowb
        d = self.dpoison[r0 * self.rowb:r0 * self.rowb + n].clone()
        rc = lib.avirhip_resize_window(
            self.p, dbig.data_ptr() + off, abi.MEM_DEVICE, a, b - a + 1,
            d.data_ptr(), abi.MEM_DEVICE, r0, r1, None)
        _ok(lib, rc, what)
        torch.cuda.synchronize()
        assert lib.avirhip_plan_get_path(self.p) == self.path, what
        return _differ(d.cpu().numpy(), self.want[r0:r1])


# ---- 1. forced chunk lengths

def _forced_runs(stages):
    """[{stage index: value}]: every knob on its own, then both together."""
    knobbed = [i for i, st in enumerate(stages) if st.knob]
    runs = [{i: v} for i in knobbed for v in stages[i].lengths]
    if len(knobbed) == 2:
        i, j = knobbed
        a, b = stages[i].lengths, stages[j].lengths
        runs += [{i: a[k % len(a)], j: b[k % len(b)]}
                 for k in range(max(len(a), len(b)))]
    return runs


def _expected_value(stages, i, run):
    """The knob value stage i runs under (AVIRHIP_SA_CHUNK rules both passes
    of the accumulation kernels, AVIRHIP_SA_CHUNK_V overrides it in the
    vertical one), None: today's rule."""
    if i in run:
        return run[i]
    for j, v in run.items():
        if (stages[j].knob == "AVIRHIP_SA_CHUNK" and
                stages[i].knob == "AVIRHIP_SA_CHUNK_V"):
            return v
    return None


def _check_line(st, x, v, problems, what):
    """One launcher line against the value its knob was given."""
    if x["field"] != st.field:
        problems.append("%s: field %s" % (what, x["field"]))
    if st.rule == "gv":
        if x["clamp"] != CC.gv_clamp(x["nt"], x["post"]):
            problems.append("%s: clamp %d with %d taps, post %d" % (
                what, x["clamp"], x["nt"], x["post"]))
    if v is not None:
        e = st.in_force(v, x.get("clamp"))
        if x["length"] != e:
            problems.append("%s: %s %d in force, %d expected" % (
                what, st.field, x["length"], e))
    if st.rows is not None and x["length"] >= 1:
        n = (st.rows + x["length"] - 1) // x["length"]
        if x["items"] != x["strips"] * n:
            problems.append("%s: %d items, %d strips x %d chunks expected" % (
                what, x["items"], x["strips"], n))


@pytest.mark.parametrize("name", CC.NAMES)
def test_whole_frame_forced_chunk_lengths(name, knob, capfd):
    n, call, stages = CC.row(name)
    knob(call[10])
    F = _Frame(call)
    # (what is printed inside the loop would be dropped with the captured
    # stderr: the notes are printed after it)
    problems, seen, notes = [], {}, []
    for run in [{}] + _forced_runs(stages):
        env = dict(call[10], AVIRHIP_VERBOSE=1)
        env.update({stages[i].knob: v for i, v in run.items()})
        knob(env)
        what = "%s %s" % (name, " ".join(
            "%s=%d" % (stages[i].knob[8:], v) for i, v in sorted(run.items()))
            or "today's rule")
        capfd.readouterr()
        diff = F.whole(what)
        lines = _lines(capfd.readouterr().err)
        if diff:
            problems.append("%s: %s" % (what, diff))
        for i, st in enumerate(stages):
            mine = _of(lines, st)
            if not mine:
                problems.append("%s: no %s line in %r" % (what, st.kernel,
                                                          lines))
            for x in mine:
                _check_line(st, x, _expected_value(stages, i, run), problems,
                            what + " " + st.kernel)
                seen.setdefault((st.kernel, st.tag), set()).add(x["length"])
                if not run:
                    notes.append("%s: %s under today's rule: %r" % (
                        name, st.kernel, x))
    print("\n".join(notes))
    for k, v in sorted(seen.items(), key=str):
        print("%s %s%s: lengths in force %s" % (name, k[0], " " + k[1] if k[1]
                                                else "", sorted(v)))
    assert not problems, "\n".join(problems[:40])


# ---- 2. every output row as a band boundary

def _band_rules(stages):
    """The environments the band walk runs under: today's rule and one forced
    length above the ring (k_lanc2 / k_lanc2h: cq 2, 10 and 26)."""
    if stages[0].rule == "cq":
        return [{"AVIRHIP_LANC2_CQ": v} for v in (2, 10, 26)]
    forced = {st.knob: st.above_ring() for st in stages if st.knob}
    return [{}] + ([forced] if forced else [])


@pytest.mark.parametrize("name", CC.NAMES)
def test_every_row_as_a_band_boundary(name, knob):
    n, call, stages = CC.row(name)
    knob(call[10])
    F = _Frame(call)
    assert not F.whole(name)
    problems = []
    for rule in _band_rules(stages):
        knob(dict(call[10], **rule))
        bad = F.cut_at_every_row("%s %r" % (name, rule))
        if bad:
            problems.append("%s under %r: bands cut at output rows %s differ"
                            % (name, rule, bad[:20]))
    assert not problems, "\n".join(problems)


# ---- 3. compact windows around seams

def _seam_bands(stages, nh):
    """(environment, three bands): a forced length above the ring; bands whose
    own grid (or, for the 2x kernels, the frame's) puts seams inside them --
    at the top edge, in the middle and at the bottom edge of the frame."""
    st = stages[-1]
    if st.rule == "cq":
        env = {"AVIRHIP_LANC2_CQ": 10}
        seams = [20 * j for j in (1, nh // 40, (nh - 1) // 20)]
        return env, [(max(0, s - 5), min(nh, s + 7)) for s in seams]
    env = {s.knob: s.above_ring() for s in stages if s.knob}
    e = st.in_force(st.above_ring(), 1 << 20) if st.knob else st.today
    h = 2 * e + 3   # two seams inside, a last chunk of three rows
    return env, [(0, h), (nh // 2 - e, nh // 2 - e + h), (nh - h, nh)]


@pytest.mark.parametrize("name", CC.NAMES)
def test_compact_windows_around_seams(name, knob):
    n, call, stages = CC.row(name)
    env, bands = _seam_bands(stages, call[4])
    knob(call[10])
    F = _Frame(call)
    knob(dict(call[10], **env))
    problems = []
    for r0, r1 in bands:
        what = "%s %r rows [%d, %d)" % (name, env, r0, r1)
        diff = F.window(r0, r1, what)
        if diff:
            problems.append("%s: %s" % (what, diff))
    assert not problems, "\n".join(problems)


# ---- 4. the double pipeline's marching kernels

def _up64_lines(err):
    lines = _lines(err)
    h = [x for x in lines if x["kernel"] == "k_uh64"]
    v = [x for x in lines if x["kernel"] == "k_uv64"]
    assert len(h) == 1 and len(v) == 1, lines
    return h[0], v[0]


@pytest.mark.parametrize("epl", CC.UP64_EPL)
@pytest.mark.parametrize("rh", CC.UP64_RH)
@pytest.mark.parametrize("name,call", CC.UP64_ROWS,
                         ids=[r[0] for r in CC.UP64_ROWS])
def test_up64_forced_chunks_bands_and_windows(name, call, rh, epl, knob,
                                              capfd):
    """k_uh64 / k_uv64 under AVIRHIP_UP64_RH x AVIRHIP_UP64_EPL: the budgets
    AVIRHIP_UP64_HB / _VW give one chunk, two, three and the shortest the
    launchers allow (4 steps of rh source rows; 48 output rows)."""
    sh, nh = call[2], call[4]
    base = {"AVIRHIP_UP64_RH": rh, "AVIRHIP_UP64_EPL": epl}
    knob(base)
    F = _Frame(call)
    knob(dict(base, AVIRHIP_VERBOSE=1))
    capfd.readouterr()
    assert not F.whole(name)
    h, v = _up64_lines(capfd.readouterr().err)
    note = "%s rh %d epl %d under today's rule: %r %r" % (name, rh, epl, h, v)
    assert (h["rh"], v["epl"]) == (rh, epl)
    problems, seen = [], set()
    for per in CC.UP64_PER_STRIP:
        hb, vw = per * h["strips"], per * v["strips"]
        knob(dict(base, AVIRHIP_VERBOSE=1, AVIRHIP_UP64_HB=hb,
                  AVIRHIP_UP64_VW=vw))
        what = "%s rh %d epl %d HB %d VW %d" % (name, rh, epl, hb, vw)
        capfd.readouterr()
        diff = F.whole(what)
        h1, v1 = _up64_lines(capfd.readouterr().err)
        if diff:
            problems.append("%s: %s" % (what, diff))
        want_h = CC.up64_crows_h(sh, h["strips"], hb, rh)
        want_v = CC.up64_crows_v(nh, v["strips"], vw)
        if (h1["length"], h1["rh"], v1["length"], v1["epl"]) != (
                want_h, rh, want_v, epl):
            problems.append("%s: %r %r, crows %d / %d expected" % (
                what, h1, v1, want_h, want_v))
        if h1["items"] != h1["strips"] * ((sh + want_h - 1) // want_h):
            problems.append("%s: %r" % (what, h1))
        seen.add((h1["length"], v1["length"]))
    print(note)
    print("%s rh %d epl %d: crows in force (h, v) %s" % (name, rh, epl,
                                                          sorted(seen)))
    # the shortest chunks: every row as a band boundary, windows around seams
    short = dict(base, AVIRHIP_UP64_HB=1000 * h["strips"],
                 AVIRHIP_UP64_VW=1000 * v["strips"])
    for rule in (base, short):
        knob(rule)
        bad = F.cut_at_every_row("%s %r" % (name, rule))
        if bad:
            problems.append("%s under %r: bands cut at output rows %s differ"
                            % (name, rule, bad[:20]))
    knob(short)
    for r0, r1 in ((0, 99), (nh // 2 - 48, nh // 2 + 51), (nh - 99, nh)):
        diff = F.window(r0, r1, "%s rows [%d, %d)" % (name, r0, r1))
        if diff:
            problems.append("%s window rows [%d, %d): %s" % (name, r0, r1,
                                                             diff))
    assert not problems, "\n".join(problems[:40])
