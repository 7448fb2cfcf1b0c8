"""The case table of tests/test_gpu_chunks.py (every marching kernel at forced
chunk lengths and at every seam) and what its host-only check,
tests/test_chunk_table.py, needs to read it.

Every fast kernel marches down a strip in chunks; a chunk's run-in, its tail
and the ring slots it hands from row to row are where these kernels can go
wrong. A family row names the call that reaches the kernel (the vocabulary of
tests/window_cases.py: front end, geometry, element types, forced path /
variant, environment) and one or two STAGES, one per marching kernel of the
call:

  kernel  the name in the library's AVIRHIP_VERBOSE line
          "<kernel>: <items> items (strips <n>, <field> <length>, ...)"
  field   "cq" (k_lanc2, k_lanc2h: source rows), "crows" (k_dnf, k_dnfh,
          k_uh64, k_uv64), "chunk" (everything else)
  knob    the variable that forces the length (None: the kernel has no knob;
          its fixed length is still read back), read per call
  rule    how the launcher turns the knob's value into the length in force
          (`in_force`): "cq" rounds up to 8k - 6 and ignores values below 2,
          "rows" clamps to the pass's rows, "clamp" to the stage's clamp,
          "gv" to the clamp the k_gv line itself reports (it depends on the tap
          count: `gv_clamp`), "none" takes the value as it is, "hb" / "vw" are
          up64.hip's rules (the knob is a work-item budget, not a length)
  rows    the rows (k_sacc's horizontal pass: outputs along x) the pass
          chunks over for the whole frame; None where it has no meaning
          (AVIR's horizontal pass runs over the source rows: all of them
          for the whole frame)
  ring    the depth of the kernel's row ring, restated from the source
  clamp   the longest chunk the launcher allows (None: no limit)
  lengths the values to force

Shapes are small: 241 (2x kernels: 242) output rows, two or three strips with
a partial last one where the planner allows it (whole-ratio downsizing plans
exist from about 96 outputs per axis on: three strips of 42 columns). 241 =
30 x 8 + 1 = 24 x 10 + 1 = 16 x 15 + 1: every row has lengths whose last
chunk is ONE row; 241 = 216 + 25: k_dnf's 4K -> 1080p height and a remainder.

The lengths real frames run at come from the host restatement of the chunk
rules below (`balanced_chunk`, `sacc_chunk`, `dnf_crows`, `lanc2_cq`) for the
README's workloads. The restatement CHOOSES INPUTS ONLY: no test compares a
length read back from the library with it. Where a rule needs plan details the
host does not have (strip widths chosen per plan, tap counts), nominal values
stand in -- 64 outputs per strip, the tap counts of the default parameter
set."""
import math
import os
import re
from avir_amd import abi

P2, P4, P5 = abi.PATH_TILED, abi.PATH_UP2, abi.PATH_GPASS
V_DN2 = abi.VARIANT_DN_TWO_PASS
V_UPG2, V_UPGF = abi.VARIANT_UPG_TWO_PASS, abi.VARIANT_UPG_FUSED
V_OPT = abi.VARIANT_SACC_OPTIMISTIC
DBL = dict(fp=abi.FPCLASS_DOUBLE)
MIN13 = {"AVIRHIP_GH2_MIN_NT": "13"}

# ---- constants restated from the sources (test_chunk_table.py parses the
# .hip files and compares)
CONSTANTS = {
    "LF_NB": 8, "LF_TE": 24,        # lfuse.hip
    "GF_NB": 8, "GF_TE": 32,        # gfuse.hip
    "GH_NB": 4,                     # gpass.hip
    "GH2_NB": 4,                    # gpass_h2.hip
    "GV_PF": 5,                     # gpass_dev.h: k_gv's ring is GV_PF + 1 deep
    "DF_W": 42,                     # dnf.hip
    "LH_MINQ": 26, "LH_RB": 8, "LH_TW": 128,   # lanc2h.hip
    "L2_RB": 8, "L2_TW": 128,       # lanc2.hip
    "SA_NS": 16,                    # sacc.hip: accumulator slots
    "U64_NT": 12, "U64_PF": 5,      # up64.hip
}
SOURCES = {"LF_NB": "lfuse.hip", "LF_TE": "lfuse.hip", "GF_NB": "gfuse.hip",
           "GF_TE": "gfuse.hip", "GH_NB": "gpass.hip", "GH2_NB": "gpass_h2.hip",
           "GV_PF": "gpass_dev.h", "DF_W": "dnf.hip", "LH_MINQ": "lanc2h.hip",
           "LH_RB": "lanc2h.hip", "LH_TW": "lanc2h.hip", "L2_RB": "lanc2.hip",
           "L2_TW": "lanc2.hip", "SA_NS": "sacc.hip", "U64_NT": "up64.hip",
           "U64_PF": "up64.hip"}
K = CONSTANTS
LF_CLAMP = K["LF_TE"] * 64 // 8     # 192 rows: 6 KiB of table
GF_CLAMP = K["GF_TE"] * 64 // 12    # 170 rows: 8 KiB of table
GV_RING = K["GV_PF"] + 1
DNF_RING = 8    # the column waves' register window of finished T rows
L2_MINQ = 58    # lanc2_run's shortest chunk of its own choice
NCU = 256


def parse_constants(csrc):
    """{name: value} of CONSTANTS' names as the sources define them."""
    out = {}
    for name, fn in SOURCES.items():
        text = open(os.path.join(csrc, fn)).read()
        m = re.search(r"^#define %s (\d+)\b" % name, text, re.M)
        assert m, "%s: no #define %s" % (fn, name)
        out[name] = int(m.group(1))
    return out


# ---- the chunk rules, restated (inputs only)

def balanced_chunk(rows, nstrips, min_chunk, max_chunk, warm, wpc, valu_bound,
                   solo=1.6):
    """gpass_dev.h: balanced_chunk."""
    cap = 256.0 * wpc
    best, best_chunk = -1.0, max(1, min(rows, max_chunk))
    min_chunk = max(1, min(min_chunk, best_chunk))
    for nch in range(1, rows + 1):
        chunk = (rows + nch - 1) // nch
        if chunk > max_chunk:
            continue
        if chunk < min_chunk:
            break
        n = (rows + chunk - 1) // chunk
        items = float(n * nstrips)
        res = math.ceil(items / cap)
        per = math.ceil(items / res / 1024.0)
        if valu_bound:
            cost = res * per * (chunk + float(warm)) * (solo if per < 2.0
                                                        else 1.0)
        else:
            cost = res * cap / items * (chunk + float(warm)) / chunk
        if best < 0.0 or cost < best:
            best, best_chunk = cost, chunk
    return best_chunk


def sacc_chunk(nout, nstrips, nt, k, lds):
    """sacc.hip: the loop of its launcher."""
    cap = 256.0 * max(1, min(16, int(160 * 1024 // (lds + 512))))
    warm = max(1.0, nt / max(1.0, k) * 0.35) + 2.0
    best, best_chunk = -1.0, nout
    for nch in range(1, nout + 1):
        chunk = (nout + nch - 1) // nch
        if chunk < 4 and nch > 1:
            break
        items = float(((nout + chunk - 1) // chunk) * nstrips)
        res = math.ceil(items / cap)
        per = math.ceil(items / res / 1024.0)
        cost = res * per * (chunk + warm) * (1.26 if per < 2.0 else 1.0)
        if best < 0.0 or cost < best:
            best, best_chunk = cost, chunk
    return best_chunk


def dnf_crows(rows, nw, ncu=NCU):
    """dnf.hip: dnf_chunk_rows without the knob."""
    nstrips = (nw + K["DF_W"] - 1) // K["DF_W"]
    want = max(1, ncu // nstrips)
    return max(8, (rows + want - 1) // want)


def cq_round(v, rb=8):
    return (v + 6 + rb - 1) // rb * rb - 6


def lanc2_cq(sh, nw, minq, tw=128):
    """lanc2.hip / lanc2h.hip: whole rounds of 256 CUs x 8 workgroups."""
    nstrips = (nw + tw - 1) // tw
    for rounds in range(1, 9):
        nch = max(1, rounds * 2048 // nstrips)
        c = cq_round((sh + nch - 1) // nch)
        if c >= minq or rounds == 8:
            return max(c, minq)


def gv_clamp(nt, post):
    """gpassv.hip: maxg - gextra (a chunk's coefficient rows fit 6 KiB)."""
    ntp = (nt + 3) & ~3
    gextra = 7 if post else 0
    return max(gextra + 1, 6144 // (ntp * 4 + 4)) - gextra


def wpc_of(lds):
    return max(1, min(16, int(160 * 1024 // (lds + 512))))


# the README's workloads: (front end, sw, sh, nw, nh)
WORKLOADS = {
    "cfg1": (640, 480, 1024, 768),
    "cfg4": (3840, 2160, 1280, 720),
    "4k_1080p": (3840, 2160, 1920, 1080),
    "1080p_2500": (1920, 1080, 2500, 1400),
    "1080p_5760": (1920, 1080, 5760, 3240),
    "photo": (5184, 3456, 1920, 1280),
}
UPSIZING = ("cfg1", "1080p_2500", "1080p_5760")
NT_AVIR_UP = 18   # IntFltLen of the default parameter set


def _strips(n, w=64):
    return (n + w - 1) // w


def real_lengths(kernel):
    """{workload: the chunk length the kernel's rule gives it} -- nominal plan
    details, see the module text."""
    out = {}
    if kernel == "k_lf":
        lds = (K["LF_NB"] * 64 + 64) * 16 + LF_CLAMP * 9 * 4 + 64
        for w in UPSIZING:
            sw, sh, nw, nh = WORKLOADS[w]
            out[w] = balanced_chunk(nh, _strips(nw), 4, LF_CLAMP, 3,
                                    wpc_of(lds), True)
    elif kernel == "k_gf":
        # (a strip's source segment of 64 pixels and its FIR output)
        lds = (K["GF_NB"] * 64 + 128) * 16 + GF_CLAMP * 13 * 4 + 64
        for w in UPSIZING:
            sw, sh, nw, nh = WORKLOADS[w]
            kv = float(sh) / nh
            warm = int(18.0 * 140.0 / (140.0 * kv + 60.0) + 0.5)
            out[w] = balanced_chunk(nh, _strips(nw), 4, GF_CLAMP, warm,
                                    wpc_of(lds), True)
    elif kernel == "k_gv":
        clamp = gv_clamp(NT_AVIR_UP, True)
        lds = (32 + 8) * 1024 + 7 * 1024 + 3072
        for w in UPSIZING:
            sw, sh, nw, nh = WORKLOADS[w]
            warm = max(1, (NT_AVIR_UP + 6) * nh // sh // 3)
            out[w] = balanced_chunk(nh, _strips(nw), 4, clamp, warm,
                                    wpc_of(lds), True)
    elif kernel in ("k_gh", "k_gh2"):
        lds = (K["GH_NB"] * 64 + 128) * 16
        for w in UPSIZING:
            sw, sh, nw, nh = WORKLOADS[w]
            out[w] = balanced_chunk(sh, _strips(nw), 4, sh, 2, wpc_of(lds),
                                    False)
    elif kernel in ("k_sacc", "k_sacc2", "k_sacc2v"):
        sw, sh, nw, nh = WORKLOADS["photo"]
        k = float(sh) / nh
        nt = int(math.ceil(NT_AVIR_UP * k))
        lds = 16 * 1024 if kernel == "k_sacc2v" else (
            0 if kernel == "k_sacc2" else 3 * 4096 + 4 * 256 + 64)
        out["photo_h"] = sacc_chunk(nw, _strips(sh), nt, k, lds)
        out["photo_v"] = sacc_chunk(nh, _strips(nw), nt, k, lds)
    elif kernel in ("k_dnf", "k_dnfh"):
        for w in ("cfg4", "4k_1080p"):
            sw, sh, nw, nh = WORKLOADS[w]
            out[w] = dnf_crows(nh, nw)
    elif kernel in ("k_lanc2", "k_lanc2h"):
        minq = L2_MINQ if kernel == "k_lanc2" else K["LH_MINQ"]
        # (exact 2x frames: cfg2's, cfg3's / cfg5's and 720p)
        for name, (sw, sh) in (("1080p_2x", (1920, 1080)),
                               ("4k_2x", (3840, 2160)),
                               ("720p_2x", (1280, 720))):
            out[name] = lanc2_cq(sh, 2 * sw, minq)
    return out


# ---- stages

class Stage(object):
    def __init__(self, kernel, field, knob, rule, rows, ring, clamp, today,
                 extra=(), tag=None):
        self.kernel, self.field, self.knob, self.rule = kernel, field, knob, rule
        self.rows, self.ring, self.clamp, self.today = rows, ring, clamp, today
        self.tag = tag      # k_sacc's pass letter in the line ("h" / "v")
        self.real = real_lengths(kernel)
        self.lengths = self._lengths(extra)

    def _lengths(self, extra):
        if self.knob is None:
            return []
        r = self.ring
        v = {1, 2, 3, self.today, r - 1, r, r + 1, 2 * r + 1}
        v.update(self.real.values())
        v.update(extra)
        if self.clamp is not None:
            v.update((self.clamp, self.clamp + 8))
        if self.rows is not None:
            v.add(self.rows)           # exactly one chunk
            if self.clamp is None:
                v.add(self.rows + 9)   # longer than the pass
        return sorted(x for x in v if x >= 1)

    def in_force(self, v, line_clamp=None):
        """The length the launcher must report for the knob's value `v`
        (None: the rule needs the line's own fields -- up64)."""
        if self.rule == "cq":
            return self.today if v < 2 else cq_round(v)
        if self.rule == "rows":
            return max(1, min(v, self.rows)) if self.rows else None
        if self.rule == "clamp":
            return max(1, min(v, self.clamp))
        if self.rule == "gv":
            return None if line_clamp is None else max(1, min(v, line_clamp))
        if self.rule == "none":
            return max(1, v)
        return None

    def chunks(self, length):
        """Chunks of the whole frame's pass at `length` rows."""
        return (self.rows + length - 1) // length

    def above_ring(self):
        """The forced value of the band and window tests: the first one whose
        length in force exceeds the ring depth."""
        for v in self.lengths:
            if self.rule == "cq" and v < 2:
                continue  # (the knob ignores it: today's length)
            e = self.in_force(v, 1 << 20)
            if e is not None and e > self.ring:
                return v
        return None


def _gh(rows, kernel="k_gh"):
    return Stage(kernel, "chunk", "AVIRHIP_GH_CHUNK", "rows", rows,
                 K["GH_NB"], None, 4)


def _gv(rows):
    # (the clamp depends on the plan's tap count: 100 is above every one)
    return Stage("k_gv", "chunk", "AVIRHIP_GV_CHUNK", "gv", rows, GV_RING,
                 None, 4, extra=(gv_clamp(NT_AVIR_UP, True),
                                 gv_clamp(6, False), 400))


def _sa(kernel, tag, rows, knob):
    return Stage(kernel, "chunk", knob, "none", rows, K["SA_NS"], None, 4,
                 tag=tag)


def _dnf(kernel="k_dnf"):
    return Stage(kernel, "crows", "AVIRHIP_DNF_CROWS", "none", 241, DNF_RING,
                 None, 8, extra=(13,))


def _l2(kernel="k_lanc2"):
    minq = L2_MINQ if kernel == "k_lanc2" else K["LH_MINQ"]
    ring = K["L2_RB"] if kernel == "k_lanc2" else K["LH_RB"]
    return Stage(kernel, "cq", "AVIRHIP_LANC2_CQ", "cq", 121, ring, None,
                 minq, extra=(26, 58, 114))


# ---- the table: (name, call, stages, extras of the test)
# call = (front end, sw, sh, nw, nh, ch, tin, tout, path, variant, env, ex);
# tin / tout are names of tests/dnf16_cases.py's T, plus "f64"

def _row(name, fe, sw, sh, nw, nh, ch, tin, tout, path, variant, stages,
         env=None, ex=None):
    return (name, (fe, sw, sh, nw, nh, ch, tin, tout, path, variant,
                   env or {}, ex or {}), stages)


UP = (64, 150, 100, 241)       # x 1.5625 / 1.607: the routes' 64x48 -> 100x77
DN3 = (300, 723, 100, 241)     # k = 3: the routes' 300x200 -> 100x67
DN22 = (254, 482, 127, 241)    # 127 = 3 x 42 + 1
DN33 = (129, 723, 43, 241)     # 43 = 42 + 1
DN23 = (254, 723, 127, 241)
X2 = (100, 121, 200, 242)      # 200 = 128 + 72

ROWS = [
    # ---- CLancIR exact 2x
    _row("lanc2_f32x4", "lancir", *X2, 4, "f32", "f32", P4, 0, [_l2()]),
    _row("lanc2_u8x4", "lancir", *X2, 4, "u8", "u8", P4, 0, [_l2()]),
    _row("lanc2_u8x3", "lancir", *X2, 3, "u8", "u8", P4, 0, [_l2()]),
    _row("lanc2h_f16", "lancir", *X2, 4, "f16", "f16", P4, 0,
         [_l2("k_lanc2h")]),
    _row("lanc2h_bf16", "lancir", *X2, 4, "bf16", "bf16", P4, 0,
         [_l2("k_lanc2h")]),
    _row("lanc2h_f16_f32", "lancir", *X2, 4, "f16", "f32", P4, 0,
         [_l2("k_lanc2h")]),
    # ---- whole-ratio downsizing
    _row("dnf_2x2", "avir", *DN22, 4, "f32", "f32", P2, 0, [_dnf()]),
    _row("dnf_3x3", "avir", *DN33, 4, "f32", "f32", P2, 0, [_dnf()]),
    _row("dnf_2x3", "avir", *DN23, 4, "f32", "f32", P2, 0, [_dnf()]),
    _row("dnfh_f16", "avir", *DN22, 4, "f16", "f16", P2, 0, [_dnf("k_dnfh")]),
    _row("dnfh_bf16_u16", "avir", *DN22, 4, "bf16", "u16", P2, 0,
         [_dnf("k_dnfh")]),
    _row("dn_two_pass", "avir", *DN22, 4, "f32", "f32", P2, V_DN2,
         [Stage("k_dnh", "chunk", None, "fixed", None, 1, None, 4),
          Stage("k_dnv", "chunk", None, "fixed", None, 1, None, 8)]),
    # ---- the pass kernels, upsizing
    _row("gh_gv_f32x4", "avir", *UP, 4, "f32", "f32", P5, V_UPG2,
         [_gh(150), _gv(241)]),
    _row("gh_gv_u8x3", "avir", *UP, 3, "u8", "u8", P5, V_UPG2,
         [_gh(150), _gv(241)]),
    _row("gh2_gv", "avir", 520, 351, 346, 241, 4, "f32", "f32", P5, 0,
         [_gh(351, "k_gh2"), _gv(241)], env=MIN13),
    _row("gf", "avir", *UP, 4, "f32", "f32", P5, V_UPGF,
         [Stage("k_gf", "chunk", "AVIRHIP_GF_CHUNK", "clamp", 241, K["GF_NB"],
                GF_CLAMP, 4)]),
    _row("lf_f32x4", "lancir", *UP, 4, "f32", "f32", P5, 0,
         [Stage("k_lf", "chunk", "AVIRHIP_LF_CHUNK", "clamp", 241, K["LF_NB"],
                LF_CLAMP, 4)]),
    # (rows of 120 bytes: a dword pitch, k_lf reads the uint8 image itself)
    _row("lf_u8x3", "lancir", 40, 93, 104, 241, 3, "u8", "u8", P5, 0,
         [Stage("k_lf", "chunk", "AVIRHIP_LF_CHUNK", "clamp", 241, K["LF_NB"],
                LF_CLAMP, 4)]),
    # ---- CLancIR downsizing: vertical pass first
    _row("lancir_dn", "lancir", *DN3, 4, "f32", "f32", P5, 0,
         [_gv(241), _gh(241)]),
    # ---- streaming accumulation (k = 3): horizontal pass (chunks of outputs
    # along x, AVIRHIP_SA_CHUNK), vertical pass (AVIRHIP_SA_CHUNK_V)
    _row("sacc_exact", "avir", *DN3, 4, "f32", "f32", P5, 0,
         [_sa("k_sacc", "h", 100, "AVIRHIP_SA_CHUNK"),
          _sa("k_sacc", "v", 241, "AVIRHIP_SA_CHUNK_V")]),
    _row("sacc2_u8x3", "avir", *DN3, 3, "u8", "u8", P5, 0,
         [_sa("k_sacc2", "h", 100, "AVIRHIP_SA_CHUNK"),
          _sa("k_sacc2v", "v", 241, "AVIRHIP_SA_CHUNK_V")]),
    _row("sacc_optimistic", "avir", *DN3, 4, "f32", "f32", P5, V_OPT,
         [_sa("k_sacc2v", "h", 100, "AVIRHIP_SA_CHUNK"),
          _sa("k_sacc2v", "v", 241, "AVIRHIP_SA_CHUNK_V")]),
]

# ---- the double pipeline's marching kernels: the knobs are work-item budgets
# (AVIRHIP_UP64_HB / _VW: a chunk is ceil(rows / (budget / strips)) rows, at
# least 4 steps of rh rows / 48 rows), so the lengths in force follow from the
# strips the line reports
UP64_ROWS = [
    ("up64_f64x4", ("avir", 50, 121, 100, 242, 4, "f64", "f64", 0, 0, {},
                    dict(DBL))),
    ("up64_f32x3", ("avir", 50, 121, 100, 242, 3, "f32", "f64", 0, 0, {},
                    dict(DBL))),
]
UP64_RH = (4, 8)
UP64_EPL = (1, 2)
# budgets per strip: one chunk, two, and as many as the floors allow
UP64_PER_STRIP = (1, 2, 3, 1000)


def up64_crows_h(rows, nstrips, hb, rh):
    want = max(1, hb // nstrips)
    c = (rows + want - 1) // want
    return max(4 * rh, (c + rh - 1) // rh * rh)


def up64_crows_v(rows, ngroups, vw):
    want = max(1, vw // ngroups)
    return max(48, (rows + want - 1) // want)


NAMES = [r[0] for r in ROWS]


def row(name):
    return ROWS[NAMES.index(name)]
