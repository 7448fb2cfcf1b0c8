"""The case table of tests/test_gpu_align.py and tests/test_align_table.py: one
row per (kernel family, form of reading the source, form of storing the
result), each with the byte alignment its fast road asks of the caller's
images -- as the launchers' predicates state it -- and the bases and pitches
that stand on either side of it.

Every fast kernel decides on the host whether it reads the caller's image
where it lies and stores into the caller's image directly; otherwise the call
steps aside: to the pack pass (a float copy of the source), to a float result
and the output stage, or -- a float RGBA call, which has neither stage -- to
the generic kernels (a FORCED path refuses such a call with
AVIRHIP_EUNSUPPORTED instead, and the automatic path serves it).

A row is a dict:
  name      its id
  files     the files of avir_amd/csrc it stands for
  fe, sw, sh, nw, nh, ch, tin, tout, bits, path, variant, ex, env
            the call, in the vocabulary of tests/far_row_cases.py
  geom2     (sw, sh, nw, nh) of the second geometry, for images whose pixels
            are no whole dwords (ch * esz no multiple of 4): source and result
            row lengths in bytes are both no multiple of 4; None otherwise --
            rows of RGBA pixels are whole dwords whatever the width
  kernel    the prefix of the family's name in the launcher's AVIRHIP_VERBOSE
            line (None: the family prints none)
  sides     src_base, src_pitch, dst_base, and dst_pitch for CLancIR
            (NewSSize) -- each a dict:
              mod    the modulus in BYTES the fast road asks (the element's
                     size where it asks no more than whole elements; 0 for
                     a pitch: packed rows and nothing else)
              where, quote
                     the file:line the predicate was read from, and its text
              aside  what takes the call otherwise, in words
              tell   how the test sees that: "refused" (the forced path
                     returns AVIRHIP_EUNSUPPORTED and leaves the destination
                     alone; the automatic path then has to serve the call),
                     "pack" / "out" (the pack pass' / the output stage's
                     AVIRHIP_VERBOSE line, which the aligned call does not
                     print), "bytes" (the plan holds a staged copy of the
                     window), None (nothing beside the road: the modulus is
                     the element's size, or it selects a store form inside
                     one stage -- the bits alone are checked)
  window    the family takes a device window where it lies (k_up2, k_lanc2,
            float RGBA); sides["window"] is the window's base
  frames    whole frames only (the error-diffusion ditherer): no bands level
  base      the stages the ALIGNED call itself shows ("pack", "out"), where
            the row pins them: a float RGB source always has the pack pass,
            an integer result of the tiles and of the ditherer the output
            stage -- and a kernel-less row (`kernel` None) whose base lacks
            "pack" thereby says that its loaders read the image raw
  note      why, at the levels the fast road admits, no load or store the
            kernel forms touches a byte outside the image's span -- written
            from the code, before the row ran

levels(row) derives the calls; on_fast_road(row, ...) says from the moduli
alone which sides of a call are on the fast road."""
import collections
from avir_amd import abi
from tests import far_row_cases as F

TYPES = F.TYPES
CSRC = F.CSRC
FILES = F.FILES
CAP = 64 << 20         # bytes a case may allocate at once
V = abi

# Levels left out, per row, with the reason in words: filled in below the
# rows (bases that are no multiple of the element size: _odd_bases).
LEFT_OUT = {}


def _side(mod, where, quote, aside, tell):
    return dict(mod=mod, where=where, quote=quote, aside=aside, tell=tell)


def _elem(esz, where, quote):
    """A side that asks whole elements and nothing more."""
    return _side(esz, where, quote, "nothing: every base / pitch of whole "
                 "elements is on the road", None)


REFUSED = ("the generic kernels (automatic path); a forced path refuses the "
           "call with AVIRHIP_EUNSUPPORTED")
PACK = "the pack pass: a float RGBA copy of the source, read instead"
OUT = "a float result and the output stage"

# ---- the predicates, once each
UP2_SRC = _side(16, "up2.hip:1781", "if( D == nullptr || ( srck == 0 && "
                "(( (uintptr_t) src & 15 ) ||", REFUSED, "refused")
UP2_PITCH = _side(16, "up2.hip:1782", "( src_stride & 3 ))) || ( io == 0 && "
                  "( (uintptr_t) dst & 7 )))", REFUSED, "refused")
UP2_DST = _side(8, "up2.hip:1782", "( src_stride & 3 ))) || ( io == 0 && "
                "( (uintptr_t) dst & 7 )))", REFUSED, "refused")
UP2_WIN = _side(16, "up2.hip:1695", "( (uintptr_t) src & 15 ) == 0 && "
                "( (uintptr_t) dst & 7 ) == 0 &&",
                "the window is copied into the plan's staging frame", "bytes")
Q_UP2_RAW = ("win.rows > 0 || ( (uintptr_t) raw & ( esz - 1 )) ||")
Q_UP2_RAW16 = ("( esz == 2 && p -> io_ch == 4 && (( (uintptr_t) raw | sb ) "
               "& 3 )) ||")
Q_UP2_IO2 = ("p -> pk_out == 65535.0 && ( (uintptr_t) iout & 1 ) == 0 ? 2 :")
Q_UP2_IO1 = ("io = ( p -> out_type == AVIRHIP_U8 && p -> tr_mul == 1.0 &&")

L2_SRC = _side(8, "lanc2.hip:608", "if( D == nullptr || ( sk == 0 && "
               "( (uintptr_t) src & 7 )) ||", REFUSED, "refused")
L2_PITCH = _side(8, "lanc2.hip:615", "( sk == 0 && (( p -> src_stride & 1 ) "
                 "||", REFUSED, "refused")
L2_DST = _side(8, "lanc2.hip:609", "( io == 0 && ( (uintptr_t) dst & 7 )) ||",
               REFUSED, "refused")
L2_DPITCH = _side(0, "lanc2.hip:500", "p -> new_stride != p -> new_w * 4 )",
                  "the plan has no k_lanc2 at all: avirhip_plan_set_path( 4 ) "
                  "refuses it, the automatic path takes the pass kernels",
                  "refused")
L2_WIN = _side(8, "lanc2.hip:565", "( (uintptr_t) src & 7 ) == 0 && "
               "( (uintptr_t) dst & 7 ) == 0 &&",
               "the window is copied into the plan's staging frame", "bytes")
Q_L2_RAW = ("( (uintptr_t) raw.ptr & ( ch == 3 ? ( type == AVIRHIP_U8 ? 0 : "
            "1 ) :")
Q_L2_RAWP = "( ch == 3 || ( raw.stride & 1 ) == 0 ) &&"
Q_DST2_U8 = "( (uintptr_t) dst & 1 ) == 0 ) &&"
Q_DST2_U16 = "( (uintptr_t) dst & ( p -> io_ch == 3 ? 1 : 3 )) == 0 ) &&"
Q_DST2_P = ("const bool dst2 = (( p -> io_ch == 3 || ( p -> new_stride & 1 ) "
            "== 0 ) &&")

GP_SRC = _side(16, "gpass.hip:2167", "( raw == nullptr && (( (uintptr_t) src "
               "& 15 ) || ( src_stride & 3 ))) ||", REFUSED, "refused")
GP_PITCH = dict(GP_SRC)
GP_DST = _side(16, "gpass.hip:2165", "if( D == nullptr || ( iout == nullptr "
               "&& ( (uintptr_t) dst & 15 )) ||", REFUSED, "refused")
GP_DPITCH = _side(16, "gpass.hip:2166", "( p -> is_lancir && ( p -> "
                  "new_stride & 3 )) ||", REFUSED, "refused")
Q_GP_RAW = "( raw != nullptr && !p -> is_lancir && !gpass_takes_raw( p )) ||"
Q_GP_U8C4 = "(( (uintptr_t) iout & 3 ) != 0 )) ||"
Q_GP_U8 = "( p -> out_type == AVIRHIP_U8 && p -> io_ch == 4 &&"
Q_GP_U16 = ("( p -> out_type == AVIRHIP_U16 && ( (uintptr_t) iout & 1 ) != 0 "
            ") ||")

FU_SRC = _side(16, "fused.hip:1038", "if( src_ch != 4 || ( (uintptr_t) src & "
               "15 ) || ( src_stride & 3 ))", REFUSED, "refused")
FU_PITCH = dict(FU_SRC)
FU_DST = _side(16, "fused.hip:1058", "if( (uintptr_t) dst & 15 )", REFUSED,
               "refused")
Q_FU_U16 = "( src_type == AVIRHIP_U16 && ( (uintptr_t) src & 1 )))"
Q_FU_RAW = "!fused_takes_raw( p, mode ) ||"
Q_TILE_OUT = "C.p -> io_ch == 4 && ( (uintptr_t) C.dst & 3 ) != 0 ) &&"
Q_EPI = "if( !rne && ech == 4 && !gamma && ( (uintptr_t) dst & 3 ) == 0 )"

Q_LF = "return( img.ptr != nullptr && ( (uintptr_t) img.ptr & 3 ) == 0 &&"
Q_LFP = "(( img.stride * esz ) & 3 ) == 0 &&"
Q_GVR = ("( (uintptr_t) img.ptr & 3 ) == 0 && (( img.stride * esz ) & 3 ) == "
         "0 &&")
Q_LSTORE = "typedef unsigned int u32u __attribute__(( aligned( 1 )));"
Q_LSTORE16 = "typedef unsigned int u32h __attribute__(( aligned( 2 )));"
Q_LOUT = ("( (uintptr_t) res & 15 ) == 0 && ( (uintptr_t) dst & ( 4 * oes - "
          "1 )) == 0 &&")

# ---- the notes, per family
N_UP2 = ("a lane DMAs the 16-byte piece that is its source pixel: with a "
         "16-byte base and pitch every piece lies inside its row, and rows "
         "and columns past the frame are clamped before the address is formed; "
         "destination half-pixels leave as 8-byte stores of two floats at "
         "8-byte addresses inside the row (row bytes are 16 * nw)")
N_UP2_RAW = ("a lane DMAs the two aligned dwords that hold its pixel and "
             "carries the base's two low bits (up2.hip:327, 422); the dwords "
             "lie in the device allocation's dword grid and the resource's "
             "range ends at the image's last byte rounded up to a dword, so "
             "only whole dwords the image shares are read (loads may read "
             "padding; nothing is stored there). Results leave through "
             "k_up2< true, IO >'s store: uint8 bytes / RGBA dwords assembled "
             "per pixel, uint16 elements whole -- each inside its row")
N_L2 = ("rows are read as 8-byte float pairs at (unsigned) sy * ss + column "
        "from an 8-byte base with an even pitch: each pair is two floats of "
        "one row; results leave as 8-byte stores inside the row")
N_L2_RAW = ("the raw loader reads the aligned word that holds a lane's RGBA "
            "pixel (2 bytes for uint8 pairs, a dword for uint16) or, for RGB, "
            "single elements; the integer stage behind a raw RGBA source "
            "stores a lane's two elements at once at their own alignment "
            "(dst2, api.cpp:979-984) and single elements otherwise: every "
            "access is whole elements of one row")
N_GP = ("float RGBA pixels travel as 16-byte LDS-DMA pieces and leave as "
        "16-byte stores: with a 16-byte base and pitch every piece is one "
        "pixel of one row, indices are clamped to the row before the address "
        "is formed")
N_GP_INT = ("the typed loaders read whole elements through a buffer resource "
            "whose range is the image (plan.h:346 image_dma_bytes), clamped "
            "to the image's last element; gp_store_int_row stores RGB uint8 "
            "quads as `aligned( 1 )` dwords made of four whole pixels of one "
            "row (gpass_dev.h:385) and keeps byte stores for a quad the row's "
            "end cuts, RGBA uint8 as one dword per pixel at a dword address, "
            "uint16 as whole elements: no store reaches past its pixel's row")
N_TILE = ("the float loader DMAs 16-byte pieces of one row from a 16-byte "
          "base and pitch; the integer loader forms element indices and "
          "clamps them to the image's last element (fused.hip:292); the "
          "tiles store float RGBA rows of the library's own result, 16-byte "
          "aligned, or the caller's float rows at a 16-byte base")
N_TILE_INT = (N_TILE + "; an integer result of the tiles (path 2 without a "
              "whole-ratio vertical kernel, path 3) is never theirs to "
              "store: fused_stores_int is false (fused.hip:1012), the float "
              "result goes through the output stage, whose per-pixel form "
              "(generic.hip:1036) stores an RGBA uint8 pixel as one dword only "
              "at a dword base and whole elements otherwise -- for these rows "
              "`the tiles' integer store` IS the generic epilogue")
N_ERRD = ("k_errd_mp stores the caller's image through eo_put / eo_flush "
          "(generic.hip:1329-1412): a lane walks ONE image row and collects "
          "its pixels' bytes in the 16-byte-aligned block of the destination "
          "they fall in, with a mask of the bytes it has written; a pixel "
          "that straddles two blocks is split (n1 < n: the first block is "
          "flushed, the rest opens the next). A block leaves as one 16-byte "
          "store only when the mask is full -- all 16 bytes are this lane's, "
          "so they are bytes of its row -- and as byte stores of exactly the "
          "masked bytes otherwise (the row's first and last blocks, the "
          "flush at p == w): no byte before the row's first or behind its "
          "last element is written, whatever the base's residue mod 16 and "
          "the row's length. The source side is the automatic path's own "
          "loaders (whole elements). The ditherer is recursive over rows: "
          "whole frames only, so the row has no bands level")
N_UP2_RGB = ("float pixels of three channels always go through the pack pass "
             "(k_pack_px indexes whole floats, generic.hip:311), k_up2 reads "
             "its 16-byte float RGBA copy; k_up2< true, 3 > stores a pixel's "
             "three floats at a dword address inside its row (up2.hip:1727 "
             "asks the dword), 12 bytes a pixel, nothing of the fourth lane")
N_DN = ("k_dnh / k_dnf read 16-byte pieces of one float row from a 16-byte "
        "base and pitch; dn_load_raw reads integer elements by a clamped "
        "element index (dn.hip:602 src_elems); the vertical kernel's integer "
        "store is gp_store_int's: bytes, whole uint16 elements or one dword "
        "per RGBA uint8 pixel at a dword address")
N_LF = ("k_lf / k_gv move integer rows as bytes by LDS-DMA: a segment starts "
        "at the dword at or below its first pixel, base and pitch are dword "
        "aligned (lfuse.hip:461-462, gpassv.hip:50) and the range is "
        "image_dma_bytes, the image rounded up to a dword inside the "
        "allocation's dword grid; gp_store_lancir_row stores uint8 pixels as "
        "`aligned( 1 )` dwords of whole pixels of one row -- whole quads of "
        "RGB pixels, byte stores for a quad the row's end cuts "
        "(gpass_dev.h:644-683) -- and uint16 RGBA as two `aligned( 2 )` "
        "dwords per pixel: nothing between CLancIR's rows is written")
N_64 = ("every element is loaded and stored whole through a 64-bit pointer "
        "sum; up64's paired stores (vec_st, up64.hip:612-613) are taken only "
        "when the base is a multiple of two elements and the row holds an "
        "even count, so a pair is two elements of one row")
N_GEN = ("the per-op kernels and the output stage index whole elements of "
         "one row; the output stage's per-pixel form (generic.hip:1036) "
         "stores an RGBA uint8 pixel as one dword only at a dword base")

F32R, U8C3, U8C4, U16C4 = F.F32R, F.U8C3, F.U8C4, F.U16C4
U16C3 = dict(ch=3, tin="u16", tout="u16", bits=16)
F64C4 = dict(ch=4, tin="f64", tout="f64", bits=16)
UPG, UPT, DN27, DN2, DN3, X2, LX2 = (F.UPG, F.UPT, F.DN27, F.DN2, F.DN3, F.X2,
                                     F.LX2)
X2T = (96, 513, 192, 1026)   # the height at which k_up2 stores integer pixels
LOWN = (128, 96, 333, 250)   # CLancIR's owner plans on the pass kernels
MIN13 = F.MIN13

ROWS = []


def _row(name, files, fe, geom, fmt, path, variant, kernel, sides, note,
         geom2=None, window=False, ex=None, env=None, frames=False,
         base=None):
    sw, sh, nw, nh = geom
    r = dict(name=name, files=list(files), fe=fe, sw=sw, sh=sh, nw=nw, nh=nh,
             path=path, variant=variant, kernel=kernel, sides=dict(sides),
             note=note, geom2=geom2, window=window, ex=dict(ex or {}),
             env=dict(env or {}), by="pitch", frames=frames,
             base=None if base is None else set(base))
    r.update(fmt)
    if fe == "lancir":
        r["bits"] = 0
    ROWS.append(r)


def _s(src_base, src_pitch, dst_base, dst_pitch=None, window=None):
    d = dict(src_base=src_base, src_pitch=src_pitch, dst_base=dst_base)
    if dst_pitch is not None:
        d["dst_pitch"] = dst_pitch
    if window is not None:
        d["window"] = window
    return d


E4 = _elem(4, "gpass.hip:2167", GP_SRC["quote"])

# ---- the per-op kernels and the generic epilogue
_row("generic_f32", ["generic.hip"], "avir", UPG, F32R, 1, 0, None,
     _s(_elem(4, "generic.hip:82", "const long so = (long) scan * a.in_ss;"),
        _elem(4, "generic.hip:82", "const long so = (long) scan * a.in_ss;"),
        _elem(4, "generic.hip:82", "const long so = (long) scan * a.in_ss;")),
     N_GEN)
for _n, _f, _g2 in (("u8c3", U8C3, (65, 48, 101, 77)), ("u8c4", U8C4, None),
                    ("u16c3", U16C3, (65, 48, 101, 77))):
    _e = TYPES[_f["tin"]][2]
    _row("generic_" + _n, ["generic.hip"], "avir", UPG, _f, 1, 0, None,
         _s(_elem(_e, "generic.hip:277", F.Q_PACK),
            _elem(_e, "generic.hip:277", F.Q_PACK),
            _side(4 if _n == "u8c4" else _e, "generic.hip:1036", Q_EPI,
                  "the element-wise form of the output stage", None)),
         N_GEN, geom2=_g2)
# ---- LDS tiles
_row("tiles_f32", ["fused.hip"], "avir", UPT, F32R, 2, 0, None,
     _s(FU_SRC, FU_PITCH, FU_DST), N_TILE)
_row("tile_fused_f32", ["fused.hip"], "avir", UPT, F32R, 3, 0, None,
     _s(FU_SRC, FU_PITCH, FU_DST), N_TILE)
for _n, _f, _g2 in (("u8c3", U8C3, (301, 200, 461, 307)), ("u8c4", U8C4, None),
                    ("u16c4", U16C4, None)):
    _e = TYPES[_f["tin"]][2]
    _row("tiles_" + _n, ["fused.hip"], "avir", UPT, _f, 2, 0, None,
         _s(_elem(_e, "fused.hip:1046", Q_FU_U16),
            _elem(_e, "fused.hip:1045", Q_FU_RAW),
            _side(4 if _n == "u8c4" else _e, "generic.hip:1036", Q_EPI,
                  "the element-wise form of the output stage", None)),
         N_TILE_INT, geom2=_g2, base=["out"])
# ---- the error-diffusion ditherer behind the automatic path: k_errd_mp
# (generic.hip:1737: padded RGBA results of w * h >= 65536), whole frames
_Q_EO = "unsigned char* const q = (unsigned char*) ( o.blk << 4 );"
for _n, _f, _g2 in (("u8c3", U8C3, (301, 200, 461, 307)), ("u8c4", U8C4, None),
                    ("u16c3", U16C3, (301, 200, 461, 307)),
                    ("u16c4", U16C4, None)):
    _e = TYPES[_f["tin"]][2]
    _row("errd_" + _n, ["generic.hip"], "avir", UPT, _f, 0, 0, None,
         _s(_elem(_e, "fused.hip:1046", Q_FU_U16),
            _elem(_e, "fused.hip:1045", Q_FU_RAW),
            _side(16, "generic.hip:1350", _Q_EO, "the same kernel: blocks a "
                  "lane fills in part leave as byte stores under its mask",
                  None)),
         N_ERRD, geom2=_g2, ex=dict(errd=1), frames=True, base=["out"])
# ---- whole-ratio downsizing: k_dnf, the two passes of dn.hip
for _n, _g in (("2", DN2), ("3", DN3)):
    _row("dnf_f32_k" + _n, ["dnf.hip"], "avir", _g, F32R, 2, 0, "k_dnf",
         _s(FU_SRC, FU_PITCH, FU_DST), N_DN)
# (k_dnf reads float RGBA rows alone, fused.hip:1072: its integer store,
# gp_store_int's, stands behind a float source)
for _n, _t, _b in (("u8c4", "u8", 8), ("u16c4", "u16", 16)):
    _row("dnf_f32_" + _n, ["dnf.hip", "fused.hip"], "avir", DN2,
         dict(ch=4, tin="f32", tout=_t, bits=_b), 2, 0, "k_dnf",
         _s(FU_SRC, FU_PITCH,
            _side(4, "api.cpp:1184", Q_TILE_OUT, OUT, "out") if _t == "u8"
            else _elem(2, "api.cpp:1184", Q_TILE_OUT)), N_DN)
_row("dn_two_pass_f32", ["dn.hip"], "avir", DN2, F32R, 2,
     V.VARIANT_DN_TWO_PASS, "k_dnv", _s(FU_SRC, FU_PITCH, FU_DST), N_DN)
for _n, _f, _g2 in (("u8c3", U8C3, (602, 400, 301, 200)), ("u8c4", U8C4, None),
                    ("u16c4", U16C4, None)):
    _e = TYPES[_f["tin"]][2]
    _row("dn_two_pass_" + _n, ["dn.hip"], "avir", DN2, _f, 2,
         V.VARIANT_DN_TWO_PASS, "k_dnv",
         _s(_elem(_e, "fused.hip:1046", Q_FU_U16),
            _elem(_e, "fused.hip:1045", Q_FU_RAW),
            _side(4, "api.cpp:1184", Q_TILE_OUT, OUT, "out")
            if _n == "u8c4" else _elem(_e, "api.cpp:1184", Q_TILE_OUT)),
         N_DN, geom2=_g2)
# ---- k_up2
_row("up2_f32", ["up2.hip"], "avir", X2, F32R, 4, 0, "k_up2",
     _s(UP2_SRC, UP2_PITCH, UP2_DST, window=UP2_WIN), N_UP2, window=True)
_row("up2_plain_f32", ["up2.hip"], "avir", X2, F32R, 4,
     V.VARIANT_UP2_PLAIN_V, "k_up2",
     _s(UP2_SRC, UP2_PITCH, UP2_DST, window=UP2_WIN), N_UP2, window=True,
     ex=dict(build_mode=1))
_row("up2_raw_u8c3", ["up2.hip"], "avir", X2T, U8C3, 4, 0, "k_up2",
     _s(_elem(1, "up2.hip:1767", Q_UP2_RAW), _elem(1, "up2.hip:1767", Q_UP2_RAW),
        _elem(1, "up2.hip:1722", Q_UP2_IO1)), N_UP2_RAW,
     geom2=(97, 513, 194, 1026))
_row("up2_raw_u8c4", ["up2.hip"], "avir", X2T, U8C4, 4, 0, "k_up2",
     _s(_elem(1, "up2.hip:1767", Q_UP2_RAW), _elem(1, "up2.hip:1767", Q_UP2_RAW),
        _elem(1, "up2.hip:1722", Q_UP2_IO1)), N_UP2_RAW)
_row("up2_raw_u16c4", ["up2.hip"], "avir", X2T, U16C4, 4, 0, "k_up2",
     _s(_side(4, "up2.hip:1768", Q_UP2_RAW16, PACK, "pack"),
        _side(4, "up2.hip:1768", Q_UP2_RAW16, PACK, "pack"),
        _elem(2, "up2.hip:1725", Q_UP2_IO2)), N_UP2_RAW)
_Q_PX = "const Tin* s = src + (long) y * src_stride + (long) x * CH;"
_row("up2_f32c3", ["up2.hip"], "avir", X2T,
     dict(ch=3, tin="f32", tout="f32", bits=16), 4, 0, "k_up2",
     _s(_elem(4, "generic.hip:311", _Q_PX), _elem(4, "generic.hip:311", _Q_PX),
        _elem(4, "up2.hip:1727", "( (uintptr_t) iout & 3 ) == 0 ? 3 :")),
     N_UP2_RGB, geom2=(97, 513, 194, 1026), base=["pack"])
# ---- the pass kernels (path 5)
_row("gpass_fused_f32", ["gfuse.hip", "gpass.hip"], "avir", UPG, F32R, 5,
     V.VARIANT_UPG_FUSED, "k_gf", _s(GP_SRC, GP_PITCH, GP_DST), N_GP)
_row("gpass_two_pass_f32", ["gpass.hip"], "avir", UPG, F32R, 5,
     V.VARIANT_UPG_TWO_PASS, "k_gv", _s(GP_SRC, GP_PITCH, GP_DST), N_GP)
_row("gpass_h2_f32", ["gpass_h2.hip", "gpass.hip"], "avir",
     (520, 300, 346, 206), F32R, 5, 0, "k_gh2", _s(GP_SRC, GP_PITCH, GP_DST),
     N_GP, env=MIN13)
_row("sacc_exact_f32", ["sacc.hip", "gpass.hip"], "avir", DN27, F32R, 5, 0,
     "k_sacc", _s(GP_SRC, GP_PITCH, GP_DST), N_GP + "; k_sacc's own test "
     "(sacc.hip:2149) asks the same 16 bytes of base and strides")
_row("sacc_optimistic_f32", ["sacc.hip", "gpass.hip"], "avir", DN27, F32R, 5,
     V.VARIANT_SACC_OPTIMISTIC, "k_sacc", _s(GP_SRC, GP_PITCH, GP_DST),
     N_GP + "; the branch-free float rows ask a dword base and pitch of "
     "their own (sacc.hip:2175), which the 16 bytes above imply")
for _n, _f, _g2 in (("u8c3", U8C3, (65, 48, 101, 77)), ("u8c4", U8C4, None),
                    ("u16c3", U16C3, (63, 48, 99, 77)),
                    ("u16c4", U16C4, None)):
    _e = TYPES[_f["tin"]][2]
    _d = (_side(4, "gpass.hip:2147", Q_GP_U8C4, OUT, "out")
          if _n == "u8c4" else
          _elem(1, "gpass.hip:2146", Q_GP_U8) if _n == "u8c3" else
          _elem(2, "gpass.hip:2148", Q_GP_U16))
    _row("gpass_gv_" + _n, ["gpass.hip", "plan.h"], "avir", UPG, _f, 5,
         V.VARIANT_UPG_TWO_PASS, "k_gv",
         _s(_elem(_e, "gpass.hip:2168", Q_GP_RAW),
            _elem(_e, "gpass.hip:2168", Q_GP_RAW), _d), N_GP_INT, geom2=_g2)
# (k_gf runs when no raw source is read, gpass.hip:1739: its integer store
# stands behind a float RGBA source)
for _n, _t, _b in (("u8c4", "u8", 8), ("u16c4", "u16", 16)):
    _row("gpass_gf_f32_" + _n, ["gfuse.hip", "gpass.hip"], "avir", UPG,
         dict(ch=4, tin="f32", tout=_t, bits=_b), 5, V.VARIANT_UPG_FUSED,
         "k_gf",
         _s(GP_SRC, GP_PITCH,
            _side(4, "gpass.hip:2147", Q_GP_U8C4, OUT, "out")
            if _t == "u8" else _elem(2, "gpass.hip:2148", Q_GP_U16)),
         N_GP + "; " + N_GP_INT)
for _n, _f, _g2 in (("u8c3", U8C3, (301, 200, 101, 67)), ("u8c4", U8C4, None),
                    ("u16c4", U16C4, None)):
    _e = TYPES[_f["tin"]][2]
    _d = (_side(4, "gpass.hip:2147", Q_GP_U8C4, OUT, "out")
          if _n == "u8c4" else
          _elem(1, "gpass.hip:2146", Q_GP_U8) if _n == "u8c3" else
          _elem(2, "gpass.hip:2148", Q_GP_U16))
    _row("sacc2_" + _n, ["sacc.hip", "gpass.hip"], "avir", DN27, _f, 5, 0,
         "k_sacc", _s(_elem(_e, "gpass.hip:2168", Q_GP_RAW),
                      _elem(_e, "gpass.hip:2168", Q_GP_RAW), _d), N_GP_INT,
         geom2=_g2)
# ---- CLancIR on the pass kernels
_row("lanc_fused_f32", ["lfuse.hip", "gpass.hip"], "lancir", UPG, F32R, 5, 0,
     "k_lf", _s(GP_SRC, GP_PITCH, GP_DST, GP_DPITCH), N_GP)
_row("lanc_two_pass_down_f32", ["gpass.hip"], "lancir", DN27, F32R, 5, 0,
     "k_gv", _s(GP_SRC, GP_PITCH, GP_DST, GP_DPITCH), N_GP)
for _n, _f, _g2 in (("u8c3", U8C3, (129, 96, 333, 250)), ("u8c4", U8C4, None),
                    ("u16c4", U16C4, None)):
    _e = TYPES[_f["tin"]][2]
    _q = Q_LSTORE16 if _n == "u16c4" else Q_LSTORE
    _w = "gpass_dev.h:622" if _n == "u16c4" else "gpass_dev.h:614"
    _row("lanc_fused_owner_" + _n, ["lfuse.hip", "plan.h"], "lancir", LOWN, _f,
         5, 0, "k_lf",
         _s(_side(4, "lfuse.hip:461", Q_LF, PACK, "pack"),
            _side(4, "lfuse.hip:462", Q_LFP, PACK, "pack"),
            _elem(_e, _w, _q), _elem(_e, _w, _q)), N_LF, geom2=_g2)
# (k_gv reads the owner's rows first, k_gh stores the owner's pixels)
for _n, _f, _g2 in (("u8c3", U8C3, (129, 96, 333, 250)), ("u8c4", U8C4, None)):
    _row("lanc_two_pass_up_owner_" + _n, ["gpass.hip", "plan.h"], "lancir",
         LOWN, _f, 5, V.VARIANT_UPG_TWO_PASS, "k_gh",
         _s(_side(4, "gpassv.hip:50", Q_GVR, PACK, "pack"),
            _side(4, "gpassv.hip:50", Q_GVR, PACK, "pack"),
            _elem(1, "gpass_dev.h:614", Q_LSTORE),
            _elem(1, "gpass_dev.h:614", Q_LSTORE)), N_LF, geom2=_g2)
_row("lanc_two_pass_down_u8c3", ["gpass.hip", "plan.h"], "lancir", DN27, U8C3,
     5, 0, "k_gv",
     _s(_side(4, "gpassv.hip:50", Q_GVR, PACK, "pack"),
        _side(4, "gpassv.hip:50", Q_GVR, PACK, "pack"),
        _elem(1, "gpass_dev.h:614", Q_LSTORE),
        _elem(1, "gpass_dev.h:614", Q_LSTORE)), N_LF,
     geom2=(301, 200, 101, 67))
# ---- k_lanc2
_row("lanc2_f32", ["lanc2.hip"], "lancir", LX2, F32R, 4, 0, "k_lanc2",
     _s(L2_SRC, L2_PITCH, L2_DST, L2_DPITCH, window=L2_WIN), N_L2,
     window=True)
_row("lanc2_raw_u8c3", ["lanc2.hip"], "lancir", LX2, U8C3, 4, 0, "k_lanc2",
     _s(_elem(1, "lanc2.hip:543", Q_L2_RAW), _elem(1, "lanc2.hip:542", Q_L2_RAWP),
        _elem(1, "api.cpp:981", Q_DST2_U8), _elem(1, "api.cpp:979", Q_DST2_P)),
     N_L2_RAW, geom2=(161, 120, 322, 240))
_row("lanc2_raw_u8c4", ["lanc2.hip"], "lancir", LX2, U8C4, 4, 0, "k_lanc2",
     _s(_side(2, "lanc2.hip:543", Q_L2_RAW, PACK, "pack"),
        _side(2, "lanc2.hip:542", Q_L2_RAWP, PACK, "pack"),
        _side(2, "api.cpp:981", Q_DST2_U8, PACK, "pack"),
        _side(2, "api.cpp:979", Q_DST2_P, PACK, "pack")), N_L2_RAW)
_row("lanc2_raw_u16c4", ["lanc2.hip"], "lancir", LX2, U16C4, 4, 0, "k_lanc2",
     _s(_side(4, "lanc2.hip:543", Q_L2_RAW, PACK, "pack"),
        _side(4, "lanc2.hip:542", Q_L2_RAWP, PACK, "pack"),
        _side(4, "api.cpp:983", Q_DST2_U16, PACK, "pack"),
        _side(4, "api.cpp:979", Q_DST2_P, PACK, "pack")), N_L2_RAW)
# ---- 8-byte elements and the double pipeline
_Q64 = "const long e = (long) y * src_stride + (long) x * CH;"
_row("lanc_f64_pack", ["generic.hip"], "lancir", LX2,
     dict(ch=4, tin="f64", tout="f64", bits=0), 0, 0, None,
     _s(_elem(8, "generic.hip:277", _Q64), _elem(8, "generic.hip:277", _Q64),
        _elem(8, "generic.hip:2306", Q_LOUT),
        _elem(8, "generic.hip:2306", Q_LOUT)), N_64)
_row("tile64_f64", ["tile64.hip"], "avir", (400, 600, 250, 375), F64C4, 0, 0,
     None, _s(*[_elem(8, "tile64.hip:282", "const Tin* const q = (const Tin*) "
                      "P.src + (long) ( row_lo + y ) *")] * 3), N_64,
     ex=dict(F.DBL, auto_path=2))
_row("generic64_f32c3", ["generic64.hip"], "avir", (400, 600, 250, 375),
     dict(ch=3, tin="f32", tout="f32", bits=16), 1, 0, None,
     _s(*[_elem(4, "generic64.hip:72", "const Tin v = src[ (long) y * "
                "src_stride + px * ch + c ];")] * 3), N_64, ex=dict(F.DBL))
_Q_VST = "( (uintptr_t) dst % ( 2 * osz )) == 0 ? 1 : 0 );"
_Q_U64 = "const Tin* const sp = (const Tin*) P.src + (long) row * P.src_ss;"
_row("up64_f32c3_f64", ["up64.hip"], "avir", (200, 400, 400, 800),
     dict(ch=3, tin="f32", tout="f64", bits=16), 0, 0, "k_uv64",
     _s(_elem(4, "up64.hip:143", _Q_U64), _elem(4, "up64.hip:143", _Q_U64),
        _side(16, "up64.hip:613", _Q_VST, "k_uv64's single-element stores",
              None)), N_64, ex=dict(F.DBL))
_row("up64_f64", ["up64.hip"], "avir", (200, 400, 400, 800), F64C4, 0, 0,
     "k_uv64",
     _s(_elem(8, "up64.hip:143", _Q_U64), _elem(8, "up64.hip:143", _Q_U64),
        _side(16, "up64.hip:613", _Q_VST, "k_uv64's single-element stores",
              None)), N_64, ex=dict(F.DBL))

NAMES = [r["name"] for r in ROWS]


def _odd_bases(r):
    """Why a row has no level with a base 1 byte off (None: its elements are
    bytes, there is no such base). The issue's bar: every access on the road
    that takes the call is byte-wise or `aligned( 1 )`, or a copy is made
    first. Each side is judged by the stage that takes an odd base there."""
    why = []
    es, ed = TYPES[r["tin"]][2], TYPES[r["tout"]][2]
    if es > 1:
        if r["tin"] == "u16" and r["ch"] != 1:
            why.append("source: every loader of uint16 rows asks an even "
                       "base (up2.hip:1767, lanc2.hip:543, fused.hip:1046, "
                       "gpassv.hip:50), so the pack pass takes it, and "
                       "k_pack_px reads four elements as one `aligned( 2 )` "
                       "64-bit word (generic.hip:299-300): legal at even "
                       "addresses only")
        else:
            why.append("source: float / double rows are read by LDS-DMA or "
                       "through `const Tin*` (k_pack_px generic.hip:311, "
                       "k_pack generic.hip:252, the per-op kernels): whole "
                       "elements at their natural alignment, no copy first")
    if ed > 1:
        if r["fe"] == "lancir" and r["tout"] == "u16":
            why.append("destination: gp_store_lancir_row stores uint16 RGBA "
                       "as `aligned( 2 )` dwords (gpass_dev.h:622) and "
                       "k_lancir_out through `Tout*`: neither is byte-wise")
        elif r["ex"].get("errd"):
            why.append("destination: eo_put itself is byte-exact at any "
                       "address, but launch_errd hands k_errd_mp a "
                       "`uint16_t*` and the single-workgroup k_errd stores "
                       "through it: the pair is not established")
        else:
            why.append("destination: the fused stores write whole elements "
                       "(gp_store_int `unsigned short*`, gpass_dev.h:239; "
                       "float / double rows as 8- and 16-byte vectors) and "
                       "ask so (up2.hip:1725-1727, gpass.hip:2148); the "
                       "output stage that takes an odd base stores through "
                       "`Tout*` (k_epilogue generic.hip:715): not byte-wise, "
                       "no copy first")
    if not why:
        return None
    return ("no base 1 byte off -- " + "; ".join(why) + ". That such an "
            "access works rests on the hardware's unaligned access mode, "
            "which the code does not establish")


for _r in ROWS:
    if _odd_bases(_r):
        LEFT_OUT[_r["name"]] = _odd_bases(_r)
SIDES = ("src_base", "src_pitch", "dst_base", "dst_pitch")


def row(name):
    return ROWS[NAMES.index(name)]


def esz_in(r):
    return TYPES[r["tin"]][2]


def esz_out(r):
    return TYPES[r["tout"]][2]


def geom(r, g):
    """(sw, sh, nw, nh) of a row's geometry 0 / 1."""
    return r["geom2"] if g else (r["sw"], r["sh"], r["nw"], r["nh"])


def at(r, g):
    """The row with the sizes of its geometry g (the call's vocabulary)."""
    q = dict(r)
    q["sw"], q["sh"], q["nw"], q["nh"] = geom(r, g)
    return q


def wants_geom2(r):
    """Pixels that are no whole dwords: rows can be no multiple of 4 bytes."""
    return (r["ch"] * esz_in(r)) % 4 != 0 or (r["ch"] * esz_out(r)) % 4 != 0


# name: its id; g: the geometry; soff / doff: bytes of the images' bases into
# their (16-byte aligned) allocations; spad / dpad: elements added to the
# source pitch / CLancIR's destination pitch; call: "frame" (one whole-frame
# avirhip_resize_band), "bands" (the bands of window_cases.bands into ONE
# image), "window" (avirhip_resize_window of the inner band, the window's base
# soff bytes in), "host" (numpy buffers, MEM_HOST)
Level = collections.namedtuple("Level", "name g soff doff spad dpad call")


def levels(r):
    es, ed = esz_in(r), esz_out(r)
    g2 = 1 if r["geom2"] else 0
    out = [Level("aligned", 0, 0, 0, 0, 0, "frame")]
    out += [Level("src+%d" % (j * es), 0, j * es, 0, 0, 0, "frame")
            for j in range(1, 16 // es)]
    out += [Level("dst+%d" % (j * ed), 0, 0, j * ed, 0, 0, "frame")
            for j in range(1, 16 // ed)]
    out += [Level("both+esz", 0, es, ed, 0, 0, "frame"),
            Level("both+16-esz", 0, 16 - es, 16 - ed, 0, 0, "frame")]
    out += [Level("pitch+%d" % e, 0, 0, 0, e, 0, "frame")
            for e in (1, 2, 3, 4, 5, 8)]
    out.append(Level("src+%d pitch+1" % es, 0, es, 0, 1, 0, "frame"))
    if r["fe"] == "lancir":
        out += [Level("dpitch+%d" % e, 0, 0, 0, 0, e, "frame")
                for e in (1, 2, 3, 4)]
    if g2:
        out.append(Level("aligned-g2", 1, 0, 0, 0, 0, "frame"))
    if not r["frames"]:
        out.append(Level("bands", g2, 0, 0, 0, 0, "bands"))
    if r["window"]:
        out += [Level("window+%d" % o, 0, o, 0, 0, 0, "window")
                for o in (0, 4, 8, 12)]
    out.append(Level("host", 0, es, ed, 0, 0, "host"))
    return out


def bands(r, g):
    """[(row0, row1)] of the `bands` level: the band list of
    tests/window_cases.py, then output rows 1, 2 and 3 on their own -- with a
    row of an odd byte count their bases are 1, 2 and 3 mod 4 between them."""
    from tests import window_cases as W
    nh = geom(r, g)[3]
    return [(a, b) for _, a, b in W.bands(nh)] + [(1, 2), (2, 3), (3, 4)]


def pitches(r, lv):
    """(source pitch, destination pitch) of a level, in elements."""
    sw, sh, nw, nh = geom(r, lv.g)
    return sw * r["ch"] + lv.spad, nw * r["ch"] + lv.dpad


def on_fast_road(r, lv, dst_off=None):
    """{side: True / False} of a call: whether it meets the side's modulus.
    dst_off: the destination base of one band (default: the level's)."""
    sp, dp = pitches(r, lv)
    v = dict(src_base=lv.soff, src_pitch=sp * esz_in(r),
             dst_base=lv.doff if dst_off is None else dst_off,
             dst_pitch=dp * esz_out(r))
    if lv.call == "window":
        return {"window": lv.soff % r["sides"]["window"]["mod"] == 0}
    pad = dict(src_pitch=lv.spad, dst_pitch=lv.dpad)
    return {s: (v[s] % r["sides"][s]["mod"] == 0 if r["sides"][s]["mod"]
                else pad[s] == 0)
            for s in SIDES if s in r["sides"]}


def tells(r, lv, dst_off=None):
    """The `tell`s a call of the level has to show: those of the sides it
    misses (empty: the fast road)."""
    return set(r["sides"][s]["tell"] for s, ok in
               on_fast_road(r, lv, dst_off).items()
               if not ok and r["sides"][s]["tell"])


def alloc_bytes(r, lv):
    """The larger of the two images of a level, with the test's margins."""
    sw, sh, nw, nh = geom(r, lv.g)
    sp, dp = pitches(r, lv)
    return max(16 + sh * sp * esz_in(r), 48 + (nh + 1) * dp * esz_out(r))


def case(r, g=0):
    """The tests/window_cases.py case of a row's geometry."""
    sw, sh, nw, nh = geom(r, g)
    return (r["fe"], sw, sh, nw, nh, r["ch"], r["tin"], r["tout"], r["bits"],
            r["path"], r["variant"], dict(r["ex"]))


def front_end(r, lv):
    """-> (front-end object, its vars / params argument) of a level."""
    from tests import window_cases as W
    if r["fe"] == "lancir":
        import avir_amd
        sp, dp = pitches(r, lv)
        return avir_amd.CLancIR(), avir_amd.CLancIRParams(
            sp if lv.spad else 0, dp if lv.dpad else 0)
    if r["ex"].get("errd"):
        import avir_amd
        obj, v = W.front_end(case(r, lv.g))
        return avir_amd.CImageResizer(r["bits"], aDitherer="errd"), v
    return W.front_end(case(r, lv.g))


def design_table():
    """DESIGN.md's table "what each family's fast road asks of the caller's
    images" (tests/test_align_table.py holds the document to it): one line
    per distinct set of moduli, in bytes (0: packed rows only); `else` names
    how a call that misses the modulus shows (the sides' `tell`)."""
    seen = collections.OrderedDict()
    for r in ROWS:
        s = r["sides"]
        key = tuple((s[k]["mod"], s[k]["where"], s[k]["tell"]) if k in s
                    else None for k in SIDES + ("window",))
        seen.setdefault(key, []).append(r["name"])
    out = []
    for key, names in seen.items():
        cells = ["--" if c is None else "%d (`%s`%s)" % (
            c[0], c[1], "" if c[2] is None else "; else " + c[2])
            for c in key]
        out.append("| %s | %s |" % (", ".join("`%s`" % n for n in names),
                                    " | ".join(cells)))
    return out
