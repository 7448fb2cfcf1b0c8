"""The case table of tests/test_gpu_far_rows.py and tests/test_far_rows_table.py:
one row per (kernel family, form of reading the source), each with the
family's own limit on how far from its base it may read -- as the code states
it -- and the row pitches that stand on either side of that limit.

The fast kernels reach their source through a buffer resource and a 32-bit
offset (row * pitch + x); whether that is safe is decided on the host, family
by family. The limits are about byte distance, not pixel count: a 64 x 48
image whose rows lie 44 MB apart ends 2 GiB from its base. These are the
smallest shapes at which that arithmetic can go wrong.

A row is a dict:
  name      its id
  files     the files of avir_amd/csrc it stands for
  fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex, env
            the call, in the vocabulary of tests/window_cases.py; tin / tout
            are names of TYPES (numpy has no bfloat16). Geometries, forced
            paths and variants are those of tests/test_gpu_bf16.py::FAMILIES,
            tests/gpass_route_cases.py and tests/window_cases.py.
  limit     expr   the quantity the family's guard bounds, a Python expression
                   of sh, sw, nh, nw, ch, esz (bytes per element) and pitch
                   (elements per row)
            op, bound, unit
                   the quantity is inside the limit while `expr op bound`
            guard  True: the host checks this and refuses (or hands the call
                   to a pack pass) beyond it. False: there is no guard,
                   because the address is formed in 64 bits or from a base
                   moved per work item -- `expr` is then the image's byte span
                   and the bound the 2 GiB a 32-bit byte offset would end at;
                   the forced path has to run at every level.
            where, quote
                   the file:line the guard (or, without one, the address
                   arithmetic) was read from, and its text
  also      further (file:line, text) pairs the note leans on
  by        "pitch": the levels are source pitches at the row's height;
            "rows": k_up2, whose pitch is capped -- the levels are heights at
            the largest admissible pitch;
            "dst": CLancIR's destination pitch (NewSSize), packed source
  window    the family takes a device window where it lies (k_up2, k_lanc2)
  note      why no address the kernel forms at the over-limit levels can leave
            the allocation -- written from the code, before the row ran

levels(row) derives from `limit`, per row:
  under     the largest pitch (height) with the quantity inside the bound
  over      the smallest with it outside
  wrap      the smallest whose byte span (rows - 1) * pitch_b + row_b exceeds
            2^32
All pitches are multiples of 16 bytes, and the test's base is 16-byte aligned,
so alignment never decides the route. A level whose allocation would exceed
CAP is dropped, and says so (Level.dropped)."""
import collections
import numpy as np
from avir_amd import abi
from tests import window_cases as W

CAP = 7 << 30          # bytes of device memory a case may hold
GIB2, GIB4 = 1 << 31, 1 << 32

# name -> (type code, numpy type of the host array, bytes per element)
TYPES = {"u8": (abi.U8, np.uint8, 1), "u16": (abi.U16, np.uint16, 2),
         "f16": (abi.F16, np.float16, 2), "bf16": (abi.BF16, np.uint16, 2),
         "f32": (abi.F32, np.float32, 4), "f64": (abi.F64, np.float64, 8)}

CSRC = "avir_amd/csrc/"
# every file a far row has to stand for (the families of the issue's table)
FILES = ["gpass.hip", "dnf.hip", "lanc2.hip", "plan.h", "sacc.hip", "up2.hip",
         "fused.hip", "dn.hip", "gfuse.hip", "lfuse.hip", "gpass_h2.hip",
         "tile64.hip", "up64.hip", "generic.hip", "generic64.hip"]
# files left out, with the reason in words (none: every file has a row)
LEFT_OUT = {}


def _lim(expr, op, bound, unit, where, quote, guard=True):
    return dict(expr=expr, op=op, bound=bound, unit=unit, where=where,
                quote=quote, guard=guard)


SPAN = "(sh - 1) * pitch * esz + sw * ch * esz"
DSPAN = "(nh - 1) * pitch * esz + nw * ch * esz"


def _none(where, quote, expr=SPAN):
    return _lim(expr, "<", GIB2, "bytes of the image's span; no guard", where,
                quote, guard=False)


L_GPASS = _lim(
    "sh * pitch * 4", "<", GIB2, "bytes, taking 4-byte elements",
    "gpass.hip:971",
    "if( (long) p -> src_h * p -> src_stride * 4 >= ( 1L << 31 ) ||")
L_DNF = _lim(
    "sh * pitch * 4", "<", 0x7fffffff, "bytes", "dnf.hip:1220",
    "if( (long) D -> v.in_len * src_ss * 4 >= 0x7fffffffL )")
L_LANC2 = _lim(
    "sh * pitch", "<", GIB2, "elements", "lanc2.hip:616",
    "(long) p -> src_h * p -> src_stride >= ( 1L << 31 ))) ||")
L_LANC2_RAW = _lim(
    "sh * pitch", "<", GIB2, "elements", "lanc2.hip:545",
    "(long) p -> src_h * raw.stride < ( 1L << 31 ));")
L_DMA = _lim(
    "((sh - 1) * pitch + sw * ch) * esz", "<=", 0x7ffffffc, "bytes",
    "plan.h:352",
    "return( bytes >= 4 && bytes <= 0x7ffffffcL ? (int) (( bytes + 3 ) & ~3L ) :")
L_UP2_PITCH = _lim(
    "pitch * 4", "<", 1 << 22, "bytes of the pitch", "up2.hip:1793",
    "if(( srck == 0 && (long) src_stride * 4 >= ( 1L << 22 )) ||")
L_UP2_RAW_PITCH = _lim(
    "pitch * esz", "<", 1 << 22, "bytes of the pitch", "up2.hip:1769",
    "sb >= ( 1L << 22 ) || getenv( \"AVIRHIP_UP2_NO_RAW\" ) != nullptr )")
L_UP2_ROWS = _none(
    "up2.hip:428",
    "const char* const sbase = (const char*) P.src + (long) ubase * srow_b;")
L_UP2_RAW_ROWS = _none(
    "up2.hip:434",
    "(int) ( rend < 0x7ffffffcL ? rend : 0x7ffffffcL ) : 0x7fffffff ),")

Q_SROW = "const int srow_b = (int) P.src_ss * 4;"
N_GPASS = ("gpass_prepare drops the pass kernels of a plan whose frame ends "
           "2 GiB or more from its base (set_path then refuses); below that "
           "every row * srow_b + x fits 31 bits, and the resource's "
           "0x7fffffff records end inside the frame's last 2 GiB")
N_DMA = ("image_dma_bytes answers 0 for an image over 0x7ffffffc bytes: the "
         "promise to read it raw is not given, the pack pass (64-bit "
         "addresses) runs; below, num_records is the image's own size and an "
         "offset past it reads zeros without touching memory")
N_64 = "the row's address is a 64-bit pointer sum; offsets within a row are small"

F32R = dict(ch=4, tin="f32", tout="f32", bits=16)
U8C3 = dict(ch=3, tin="u8", tout="u8", bits=8)
U8C4 = dict(ch=4, tin="u8", tout="u8", bits=8)
U16C4 = dict(ch=4, tin="u16", tout="u16", bits=16)
DBL = dict(fp=abi.FPCLASS_DOUBLE)
MIN13 = {"AVIRHIP_GH2_MIN_NT": "13"}
V = abi

ROWS = []


def _row(name, files, fe, geom, fmt, path, variant, limit, note, also=(),
         by="pitch", window=False, ex=None, env=None):
    sw, sh, nw, nh = geom
    r = dict(name=name, files=list(files), fe=fe, sw=sw, sh=sh, nw=nw, nh=nh,
             path=path, variant=variant, limit=limit, note=note,
             also=list(also), by=by, window=window, ex=dict(ex or {}),
             env=dict(env or {}))
    r.update(fmt)
    if fe == "lancir":
        r["bits"] = 0
    ROWS.append(r)


UPG = (64, 48, 100, 77)      # upsizing, general ratio
UPT = (300, 200, 460, 307)   # ... at the tiles' size
DN27 = (300, 200, 100, 67)   # 3x down: the accumulation kernels
DN2 = (600, 400, 300, 200)   # whole ratio 2
DN3 = (600, 402, 200, 134)   # whole ratio 3
X2 = (96, 70, 192, 140)      # exact 2x
LX2 = (160, 120, 320, 240)   # ... CLancIR's

# ---- the per-op kernels
_row("generic_f32", ["generic.hip"], "avir", UPG, F32R, 1, 0,
     _none("generic.hip:82", "const long so = (long) scan * a.in_ss;"), N_64)
# ---- LDS tiles
N_TILE = ("the resource is based at the tile row's own address (64-bit), its "
          "offsets stay within the row")
_row("tiles_f32", ["fused.hip"], "avir", UPT, F32R, 2, 0,
     _none("fused.hip:405", "(const float*) P.src + (long) gy * P.src_ss ), 0,"),
     N_TILE)
_row("tile_fused_f32", ["fused.hip"], "avir", UPT, F32R, 3, 0,
     _none("fused.hip:405", "(const float*) P.src + (long) gy * P.src_ss ), 0,"),
     N_TILE)
for _n, _f in (("u8c3", U8C3), ("u16c4", U16C4)):
    _row("tiles_" + _n, ["fused.hip"], "avir", UPT, _f, 2, 0,
         _none("fused.hip:297", "const long row_e = (long) gy * P.src_ss;"),
         "the integer loader forms element indices in long and clamps them "
         "to the image's last element (fused.hip:292)",
         also=[("fused.hip:292", "const long total = (long) ( P.src_h - 1 ) "
                "* P.src_ss + (long) P.src_w * ch;")])
# ---- whole-ratio downsizing: k_dnf, and the two passes of dn.hip
for _n, _g in (("2", DN2), ("3", DN3)):
    _row("dnf_f32_k" + _n, ["dnf.hip"], "avir", _g, F32R, 2, 0, L_DNF,
         "dn_run_hv returns 1 before it launches and the two passes of "
         "dn.hip (a base per row) run; below the limit every row offset "
         "fits 31 bits under a 0x7fffffff range based at the frame")
_row("dn_two_pass_f32", ["dn.hip"], "avir", DN2, F32R, 2,
     V.VARIANT_DN_TWO_PASS,
     _none("dn.hip:220", "(void*) ( (const float*) P.src + (long) y * P.src_ss ), 0,"),
     "k_dnh bases its resource at the row it reads (64-bit); the vertical "
     "pass reads the packed FltBuf")
for _n, _f in (("u8c3", U8C3), ("u16c4", U16C4)):
    _row("dn_two_pass_" + _n, ["dn.hip"], "avir", DN2, _f, 2,
         V.VARIANT_DN_TWO_PASS,
         _none("dn.hip:239", "dn_load_raw< uint8_t, NDMA >( (const uint8_t*) "
               "P.src, (long) y *"),
         "the raw loader takes its row's element index as a long and is "
         "bounded by src_elems, a long (dn.hip:602)",
         also=[("dn.hip:602", "P.src_elems = (long) ( b - 1 ) * src_ss + "
                "(long) D -> h.in_len * src_ch;")])
# ---- k_up2: the pitch is capped; rows beyond 2 GiB are reached by height
N_UP2 = ("each work item bases its resource at its own first row (64-bit) and "
         "reads at most 512 rows of a pitch below 4 MiB from there: offsets "
         "stay below 2^31 whatever the frame's height")
_row("up2_f32_pitch", ["up2.hip"], "avir", X2, F32R, 4, 0, L_UP2_PITCH,
     "up2_run returns 1 for a pitch of 4 MiB or more, before it launches",
     window=True)
_row("up2_f32_rows", ["up2.hip"], "avir", X2, F32R, 4, 0, L_UP2_ROWS, N_UP2,
     by="rows", window=True)
_row("up2_plain_f32_rows", ["up2.hip"], "avir", X2, F32R, 4,
     V.VARIANT_UP2_PLAIN_V, L_UP2_ROWS, N_UP2, by="rows", window=True,
     ex=dict(build_mode=1))
# (513 rows: the height at which the uint8 plan is known to take the raw road,
# up2_raw_u8c4_rows' `under`; the 70-row plan runs the plain form behind the
# pack pass whatever the pitch)
_row("up2_raw_u8c4_pitch", ["up2.hip"], "avir", (96, 513, 192, 1026), U8C4, 4,
     0, L_UP2_RAW_PITCH,
     "up2_run refuses the raw image at a pitch of 4 MiB or more; the pack "
     "pass (64-bit addresses) makes the float copy the kernel then reads")
for _n, _f in (("u8c4", U8C4), ("u8c3", U8C3), ("u16c4", U16C4),
               ("f16c4", dict(ch=4, tin="f16", tout="f16", bits=16)),
               ("bf16c4", dict(ch=4, tin="bf16", tout="bf16", bits=16))):
    _row("up2_raw_%s_rows" % _n, ["up2.hip"], "avir", X2, _f, 4, 0,
         L_UP2_RAW_ROWS,
         N_UP2 + "; the raw range (num_records) is the image's end seen from "
         "that base, computed in long and stopped at 0x7ffffffc -- as an int "
         "product it wrapped for frames of 2 GiB and the rows behind the "
         "wrapped end read as zeros",
         by="rows",
         also=[("up2.hip:430", "const long rend = ( rsh + (long) ( P.rmax - "
                "ubase ) * srow_b +")])
# ---- the pass kernels (path 5): one guard in gpass_prepare for all of them
_row("gpass_fused_f32", ["gfuse.hip", "gpass.hip"], "avir", UPG, F32R, 5,
     V.VARIANT_UPG_FUSED, L_GPASS, N_GPASS, also=[("gfuse.hip:202", Q_SROW)])
_row("gpass_two_pass_f32", ["gpass.hip"], "avir", UPG, F32R, 5,
     V.VARIANT_UPG_TWO_PASS, L_GPASS, N_GPASS,
     also=[("gpass.hip:98", Q_SROW)])
_row("gpass_two_pass_u8c3", ["gpass.hip", "plan.h"], "avir", UPG, U8C3, 5, 0,
     L_GPASS, N_GPASS + "; the guard takes 4-byte elements, so for uint8 rows "
     "it refuses at a quarter of the distance the DMA's own range "
     "(image_dma_bytes) would allow",
     also=[("plan.h:352", L_DMA["quote"])])
_row("gpass_h2_f32", ["gpass_h2.hip", "gpass.hip"], "avir",
     (520, 300, 346, 206), F32R, 5, 0, L_GPASS, N_GPASS, env=MIN13,
     also=[("gpass_h2.hip:98", Q_SROW)])
Q_SACC = "hrow[ k ] = min( l0 + k * 16 + ( lane >> 2 ), llast ) * slane;"
N_SACC = N_GPASS + ("; k_sacc's int product row * slane (bytes) is a row "
                    "offset of the same frame")
_row("sacc_exact_f32", ["sacc.hip", "gpass.hip"], "avir", DN27, F32R, 5, 0,
     L_GPASS, N_SACC, also=[("sacc.hip:293", Q_SACC)])
_row("sacc_optimistic_f32", ["sacc.hip", "gpass.hip"], "avir", DN27, F32R, 5,
     V.VARIANT_SACC_OPTIMISTIC, L_GPASS, N_SACC + "; the branch-free form "
     "asks s_lane * lane_hi < 2^31 of its own (sacc.hip:2176)",
     also=[("sacc.hip:2176", "(double) s_lane * lane_hi < 2147483648.0 ))) ||")])
for _n, _f in (("u8c3", U8C3), ("u16c4", U16C4)):
    _row("sacc2_" + _n, ["sacc.hip", "gpass.hip"], "avir", DN27, _f, 5, 0,
         L_GPASS, N_SACC + "; integer rows are 1 or 2 bytes an element, the "
         "guard takes 4: it refuses early, never late")
# ---- CLancIR on the pass kernels
_row("lanc_fused_f32", ["lfuse.hip", "gpass.hip"], "lancir", UPG, F32R, 5, 0,
     L_GPASS, N_GPASS, also=[("lfuse.hip:116", "const int srow_b = ( RAW ? "
                              "(int) P.raw_ss * ( raw_kind == 1 ? 1 :")])
for _n, _f in (("u8c3", U8C3), ("u16c4", U16C4)):
    _row("lanc_fused_owner_" + _n, ["lfuse.hip", "plan.h"], "lancir",
         (128, 96, 333, 250), _f, 5, 0, L_DMA, N_DMA,
         also=[("lfuse.hip:463",
                "image_dma_bytes( img, in_len_v, width ) != 0 &&")])
_row("lanc_two_pass_up_f32", ["gpass.hip"], "lancir", UPG, F32R, 5,
     V.VARIANT_UPG_TWO_PASS, L_GPASS, N_GPASS)
_row("lanc_two_pass_down_f32", ["gpass.hip"], "lancir", DN27, F32R, 5, 0,
     L_GPASS, N_GPASS)
_row("lanc_two_pass_down_u8c3", ["gpass.hip", "plan.h"], "lancir", DN27, U8C3,
     5, 0, L_DMA, N_DMA,
     also=[("gpassv.hip:51", "image_dma_bytes( img, A.in_len, width ) != 0 &&")])
# ---- k_lanc2: a 32-bit ELEMENT offset, zero-extended
N_LANC2 = ("the kernel forms (unsigned) sy * (unsigned) ss + column, a 32-bit "
           "element index that cannot wrap below the limit, and adds it to a "
           "64-bit pointer; lanc2_run returns 1 beyond the limit")
_row("lanc2_f32", ["lanc2.hip"], "lancir", LX2, F32R, 4, 0, L_LANC2, N_LANC2,
     window=True,
     also=[("lanc2.hip:220", "pre[ r ] = *(const f2*) ( P.src + ( (unsigned) "
            "sy *")])
for _n, _f in (("u8c4", U8C4), ("u8c3", U8C3), ("u16c4", U16C4)):
    _row("lanc2_raw_" + _n, ["lanc2.hip"], "lancir", LX2, _f, 4, 0,
         L_LANC2_RAW, N_LANC2 + " (the pack pass then makes the float copy)",
         also=[("lanc2.hip:185", "( (unsigned) sy * (unsigned) P.raw_ss + "
                "rcol );")])
# ---- 8-byte elements: CLancIR's raw rows, and the double pipeline
N_F64 = ("double rows are read by the pack pass alone (lanc_road: in_fast "
         "is false), one 64-bit address per pixel")
Q_PACK = "const long e = (long) y * src_stride + (long) x * CH;"
_row("lanc_f64_pack", ["generic.hip"], "lancir", LX2,
     dict(ch=4, tin="f64", tout="f64", bits=0), 0, 0,
     _none("generic.hip:277", Q_PACK),
     N_F64)
_row("lanc_f64_pack_c3", ["generic.hip"], "lancir", UPG,
     dict(ch=3, tin="f64", tout="f64", bits=0), 0, 0,
     _none("generic.hip:277", Q_PACK), N_F64)
_row("tile64_f64", ["tile64.hip"], "avir", (400, 600, 250, 375),
     dict(ch=4, tin="f64", tout="f64", bits=16), 0, 0,
     _none("tile64.hip:282", "const Tin* const q = (const Tin*) P.src + "
           "(long) ( row_lo + y ) *"), N_64, ex=dict(DBL, auto_path=2))
_row("generic64_f32c3", ["generic64.hip"], "avir", (400, 600, 250, 375),
     dict(ch=3, tin="f32", tout="f32", bits=16), 1, 0,
     _none("generic64.hip:72", "const Tin v = src[ (long) y * src_stride + "
           "px * ch + c ];"), N_64, ex=dict(DBL))
_row("up64_f32c3_f64", ["up64.hip"], "avir", (200, 400, 400, 800),
     dict(ch=3, tin="f32", tout="f64", bits=16), 0, 0,
     _none("up64.hip:143", "const Tin* const sp = (const Tin*) P.src + "
           "(long) row * P.src_ss;"), N_64, ex=dict(DBL))
_row("up64_f64", ["up64.hip"], "avir", (200, 400, 400, 800),
     dict(ch=4, tin="f64", tout="f64", bits=16), 0, 0,
     _none("up64.hip:143", "const Tin* const sp = (const Tin*) P.src + "
           "(long) row * P.src_ss;"), N_64, ex=dict(DBL))

# ---- CLancIR's destination pitch (NewSSize), packed source. (The avir
# description has no destination pitch.) Every store is a 64-bit address.
N_DST = ("the store's address is a 64-bit pointer sum of (long) row * pitch; "
         "nothing between the rows is written")
_row("dst_lanc_fused_f32", ["lfuse.hip"], "lancir", UPG, F32R, 5, 0,
     _none("lfuse.hip:239", "float* dp = P.dst + (long) ( y0 - P.dst_row0 ) * "
           "P.dst_ss + (long) j * 4;", DSPAN), N_DST, by="dst")
_row("dst_lanc_two_pass_f32", ["gpass.hip"], "lancir", DN27, F32R, 5, 0,
     _none("gpass.hip:399", "*(f4*) ( P.dst + (long) ( r - P.dst_row0 ) * "
           "P.dst_ss +", DSPAN), N_DST, by="dst")
_row("dst_lanc_fused_owner_u8c3", ["gpass_dev.h"], "lancir",
     (128, 96, 333, 250), U8C3, 5, 0,
     _none("gpass_dev.h:222", "unsigned char* const p = (unsigned char*) "
           "O.base + row * O.stride +", DSPAN),
     N_DST + " (O.stride is a long)", by="dst")
_row("dst_lanc2_owner_u8c4", ["lanc2.hip"], "lancir", LX2, U8C4, 4, 0,
     _none("lanc2.hip:354", "const long ro = (long) ( y - P.dst_row0 ) * "
           "P.istride;", DSPAN), N_DST, by="dst")
_row("dst_lanc_generic_f32", ["generic.hip"], "lancir", UPG, F32R, 1, 0,
     _none("generic.hip:2125", "const long rstride = ( direct ? (long) p -> "
           "new_stride :", DSPAN), N_DST, by="dst")
_row("dst_lanc_f64", ["generic.hip"], "lancir", LX2,
     dict(ch=4, tin="f64", tout="f64", bits=0), 0, 0,
     _none("generic.hip:2125", "const long rstride = ( direct ? (long) p -> "
           "new_stride :", DSPAN), N_DST, by="dst")

NAMES = [r["name"] for r in ROWS]
LEVELS = ("under", "over", "wrap")

# the family groups of tests/test_gpu_far_rows.py (one floor each), by the
# rows' name prefixes; the first match holds
_GROUPS = [("dst_", "lancir_destination"), ("up2_", "up2"),
           ("lanc2_", "lanc2"), ("lanc_f64", "eight_byte"),
           ("tile64", "eight_byte"), ("generic64", "eight_byte"),
           ("up64", "eight_byte"), ("lanc_", "lancir_pass_kernels"),
           ("gpass_", "avir_pass_kernels"), ("sacc", "avir_pass_kernels"),
           ("dn", "whole_ratio_down"), ("generic_", "tiles_and_per_op"),
           ("tile", "tiles_and_per_op")]
for _r in ROWS:
    _r["group"] = [g for p_, g in _GROUPS if _r["name"].startswith(p_)][0]
GROUPS = sorted(set(r["group"] for r in ROWS))


def group(name):
    return [r for r in ROWS if r["group"] == name]


def row(name):
    return ROWS[NAMES.index(name)]


def esz_of(r):
    """Bytes per element of the image the levels move apart."""
    return TYPES[r["tout" if r["by"] == "dst" else "tin"]][2]


def quantity(r, pitch, sh=None):
    """The guarded quantity of a row at `pitch` elements (and height sh)."""
    sh = r["sh"] if sh is None else sh
    nh = r["nh"] if r["by"] != "rows" else 2 * sh
    return eval(r["limit"]["expr"], {"__builtins__": {}}, dict(
        sh=sh, sw=r["sw"], nh=nh, nw=r["nw"], ch=r["ch"], esz=esz_of(r),
        pitch=pitch))


def inside(r, pitch, sh=None):
    q, b = quantity(r, pitch, sh), r["limit"]["bound"]
    return q < b if r["limit"]["op"] == "<" else q <= b


def span(r, pitch, sh=None):
    """Bytes from the image's first to behind its last element."""
    if r["by"] == "dst":
        rows, width = r["nh"], r["nw"]
    else:
        rows, width = (r["sh"] if sh is None else sh), r["sw"]
    return ((rows - 1) * pitch + width * r["ch"]) * esz_of(r)


Level = collections.namedtuple(
    "Level", "name sh pitch inside alloc dropped")


def _largest(ok, lo, hi):
    """The largest v in [lo, hi] with ok(v); ok is true at lo, monotone."""
    assert ok(lo)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


def levels(r):
    """-> [Level]: under, over, wrap (see the module's text)."""
    es = esz_of(r)
    q = 16 // es                      # pitch granule: 16 bytes
    out = []
    if r["by"] == "rows":
        # the largest admissible pitch: 16 bytes below 4 MiB
        pitch = ((1 << 22) - 16) // es
        hmax = 1 << 16
        under = _largest(lambda h: inside(r, pitch, h), 2, hmax)
        wrap = _largest(lambda h: span(r, pitch, h) <= GIB4, 2, hmax) + 1
        for name, sh in (("under", under), ("over", under + 1),
                         ("wrap", wrap)):
            out.append((name, sh, pitch))
    else:
        width = (r["nw"] if r["by"] == "dst" else r["sw"]) * r["ch"]
        lo = (width + q - 1) // q     # in granules
        hi = (2 ** 31 - 1) // q
        under = _largest(lambda g: inside(r, g * q), lo, hi) * q
        wrap = (_largest(lambda g: span(r, g * q) <= GIB4, lo, hi) + 1) * q
        for name, pitch in (("under", under), ("over", under + q),
                            ("wrap", wrap)):
            out.append((name, r["sh"], pitch))
    res = []
    for name, sh, pitch in out:
        alloc = span(r, pitch, sh)
        res.append(Level(name, sh, pitch, inside(r, pitch, sh), alloc,
                         "needs %.2f GiB, the cap is %d GiB" % (
                             alloc / 2.0 ** 30, CAP >> 30)
                         if alloc + (64 << 20) > CAP else None))
    return res


def level(r, name):
    return levels(r)[LEVELS.index(name)]


def case(r, lv):
    """The tests/window_cases.py case of a row at a level."""
    ex = dict(r["ex"])
    sh, nh = lv.sh, (2 * lv.sh if r["by"] == "rows" else r["nh"])
    return (r["fe"], r["sw"], sh, r["nw"], nh, r["ch"], r["tin"], r["tout"],
            r["bits"], r["path"], r["variant"], ex)


def front_end(r, lv):
    """-> (front-end object, its vars / params argument) with the level's
    pitch: SrcScanlineSize is the avir plan's own argument."""
    c = case(r, lv)
    if r["fe"] == "lancir":
        import avir_amd
        P = (avir_amd.CLancIRParams(0, lv.pitch) if r["by"] == "dst" else
             avir_amd.CLancIRParams(lv.pitch, 0))
        return avir_amd.CLancIR(), P
    return W.front_end(c)


def design_table():
    """The rows of DESIGN.md's table "how far from its base each family may
    read, and who checks" (tests/test_far_rows_table.py holds the document
    to it): one per guard, and one for all the places that need none."""
    guards, free = collections.OrderedDict(), []
    for r in ROWS:
        l = r["limit"]
        if not l["guard"]:
            if l["where"] not in free:
                free.append(l["where"])
            continue
        g = guards.setdefault(l["where"], (l, []))
        g[1].extend(f for f in r["files"] if f not in g[1])
    out = ["| %s | `%s` | `%s %s %#x` %s | the host: refuses, or packs first |"
           % (", ".join("`%s`" % f for f in fs), w, l["expr"], l["op"],
              l["bound"], l["unit"]) for w, (l, fs) in guards.items()]
    out.append("| %s | -- | any distance: a 64-bit address per row, or a base "
               "moved per work item | nobody has to |" % ", ".join(
                   "`%s`" % w for w in free))
    return out
