"""avir_amd -- MI355X-native executor for the separable-resize hot path of
avaneev/avir, behind the reference's own front-end API.

`CImageResizer` mirrors avir::CImageResizer<> (avir.h:4609-5092) and `CLancIR`
mirrors avir::CLancIR (lancir.h:327-755): same constructor arguments, same
`resizeImage` argument order and meaning, same error behaviour. Both are thin
ctypes shells over the C ABI of libavirhip.so (include/avirhip.h); the
arithmetic runs in hand-written HIP kernels on gfx950. There is no CPU
fallback: without the built library or without a GPU the calls raise.

Buffers may be numpy arrays (host memory; staged through the device inside the
call) or torch CUDA tensors (device memory; zero-copy, asynchronous on the
current torch stream).
"""
import ctypes as C
import numpy as np

from . import abi
from .abi import AvirHipError, U8, U16, F32, F64, U32, F16, BF16

__all__ = ["CImageResizer", "CImageResizerParams", "CImageResizerVars",
           "CLancIR", "CLancIRParams", "AvirHipError", "device_count"]

_NP2T = {np.dtype(np.uint8): U8, np.dtype(np.uint16): U16,
         np.dtype(np.float32): F32, np.dtype(np.float64): F64,
         # CLancIR only ("treated as uint16_t", lancir.h:376-377); CImageResizer
         # refuses it like the reference's unsupported types
         np.dtype(np.uint32): U32,
         np.dtype(np.float16): F16}


def device_count():
    return abi.load().avirhip_device_count()


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class _on_device_of(object):
    """Makes the device of the first CUDA tensor among `bufs` current for the
    duration of a call: plans, scratch and the cache key belong to the device
    that is current when the library is entered."""

    def __init__(self, *bufs):
        self.ctx = None
        for b in bufs:
            if _is_torch(b) and b.is_cuda:
                import torch
                self.ctx = torch.cuda.device(b.device)
                break

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def _numel(x):
    return int(x.numel()) if _is_torch(x) else int(x.size)


def _need(x, n, what):
    """A short buffer would become a silent out-of-bounds copy or device
    write inside the library: refuse it here."""
    if _numel(x) < n:
        raise ValueError("%s holds %d elements, the call needs %d"
                         % (what, _numel(x), n))


def _torch_dtype_code(x):
    import torch
    tmap = {torch.uint8: U8, torch.float32: F32, torch.float64: F64,
            torch.float16: F16, torch.bfloat16: BF16}
    if hasattr(torch, "uint16"):
        tmap[torch.uint16] = U16
    if hasattr(torch, "uint32"):
        tmap[torch.uint32] = U32
    return tmap[x.dtype]


def _buf(x):
    """-> (pointer, mem kind, dtype code, stream)"""
    if _is_torch(x):
        import torch
        if not x.is_contiguous():
            raise ValueError("tensor must be contiguous")
        if x.is_cuda:
            st = torch.cuda.current_stream(x.device).cuda_stream
            return x.data_ptr(), abi.MEM_DEVICE, _torch_dtype_code(x), st
        return x.data_ptr(), abi.MEM_HOST, _torch_dtype_code(x), None
    a = x
    if not isinstance(a, np.ndarray) or not a.flags["C_CONTIGUOUS"]:
        raise ValueError("buffer must be a C-contiguous numpy array or a "
                         "contiguous torch tensor")
    return a.ctypes.data, abi.MEM_HOST, _NP2T[a.dtype], None


class _Views(object):
    """One side of a planar call as plane views (abi.PlaneView, include/
    avirhip.h "Plane views"): the host array, the element type, the stream and
    the tensors it points into. The library reads the array inside the call."""

    def __init__(self, table, dt, stream, keep):
        self.table = np.ascontiguousarray(table, dtype=np.int64)
        self.count = int(self.table.shape[0])
        self.ptr, self.dt, self.stream, self.keep = (
            self.table.ctypes.data, dt, stream, keep)

    @staticmethod
    def _check(x, what):
        if not (_is_torch(x) and x.is_cuda):
            raise ValueError("%s: plane views take CUDA tensors (host memory "
                             "behind a view is not supported)" % what)

    @classmethod
    def of_planes(cls, planes, w, h, what):
        """A sequence of per-plane (H, W) CUDA tensors, each with its own
        base, row stride and element stride."""
        import torch
        if len(planes) == 0:
            raise ValueError("%s: no planes" % what)
        rows = []
        for t in planes:
            cls._check(t, what)
            if (tuple(t.shape) != (h, w) or t.dtype != planes[0].dtype
                    or t.device != planes[0].device):
                raise ValueError("%s: every plane must be a (%d, %d) tensor "
                                 "of one dtype on one device" % (what, h, w))
            sy, sx = (int(n) for n in t.stride())
            if (h > 1 and sy < 1) or (w > 1 and sx < 1):
                raise ValueError("%s: positive strides are required" % what)
            rows.append((t.data_ptr(), sy if h > 1 else 0,
                         sx if w > 1 else 1))
        st = torch.cuda.current_stream(planes[0].device).cuda_stream
        return cls(np.array(rows, dtype=np.int64).reshape(-1, 3),
                   _torch_dtype_code(planes[0]), st, list(planes))

    @classmethod
    def of_tensor(cls, x, what):
        """A (..., H, W) CUDA tensor with any positive strides: one view per
        index of the leading dimensions, in C order."""
        import torch
        cls._check(x, what)
        h, w = int(x.shape[-2]), int(x.shape[-1])
        sy, sx = int(x.stride(-2)), int(x.stride(-1))
        lead = [int(n) for n in x.shape[:-2]]
        lstr = [int(n) for n in x.stride()[:-2]]
        if ((h > 1 and sy < 1) or (w > 1 and sx < 1)
                or any(n > 1 and q < 1 for n, q in zip(lead, lstr))):
            raise ValueError("%s: positive strides are required" % what)
        offs = np.zeros((1,), np.int64)
        for n, q in zip(lead, lstr):
            offs = (offs[:, None] + np.arange(n, dtype=np.int64)[None, :] * q
                    ).reshape(-1)
        tab = np.empty((offs.size, 3), np.int64)
        tab[:, 0] = x.data_ptr() + offs * x.element_size()
        tab[:, 1] = sy if h > 1 else 0
        tab[:, 2] = sx if w > 1 else 1
        st = torch.cuda.current_stream(x.device).cuda_stream
        return cls(tab, _torch_dtype_code(x), st, x)


def _plane_side(x, w, h, what):
    """One side of a planar call -> (pointer, mem kind, dtype code, stream,
    views or None): a buffer as _buf takes it, or a sequence of per-plane
    (H, W) CUDA tensors, which become plane views."""
    if isinstance(x, (list, tuple)):
        x = _Views.of_planes(x, w, h, what)
    if isinstance(x, _Views):
        return x.ptr, abi.MEM_VIEWS, x.dt, x.stream, x
    return _buf(x) + (None,)


def _device_of(x):
    """The tensor a planar call's device is taken from."""
    if isinstance(x, _Views):
        x = x.keep
    if isinstance(x, (list, tuple)):
        x = x[0]
    return x


def _planes_operands(src, NewWidth, NewHeight, out_dtype, out):
    """resize_planes' two sides -> (SrcBuf, NewBuf, result, h, w, n): today's
    contiguous path where both are contiguous, plane views where a CUDA
    tensor is not -- never a hidden copy."""
    if len(src.shape) < 2:
        raise ValueError("resize_planes: (..., H, W) expected")
    lead = tuple(int(n) for n in src.shape[:-2])
    h, w = int(src.shape[-2]), int(src.shape[-1])
    n = 1
    for d in lead:
        n *= d
    shape = lead + (NewHeight, NewWidth)
    if out is not None and tuple(out.shape) != shape:
        raise ValueError("resize_planes: out must have the shape %r"
                         % (shape,))
    if out is not None and _is_torch(out) != _is_torch(src):
        raise ValueError("resize_planes: src and out must both be torch "
                         "tensors or both numpy arrays")
    if not _is_torch(src):
        dst = out if out is not None else np.empty(shape,
                                                   out_dtype or src.dtype)
        return src, dst, dst, h, w, n
    import torch
    if out is None:
        if src.is_contiguous():
            out = torch.empty(shape, device=src.device,
                              dtype=out_dtype or src.dtype)
        else:
            # the source's memory format: dense in its order of dimensions
            order = sorted(range(len(shape)),
                           key=lambda d: (-int(src.stride(d)), d))
            out = torch.empty([shape[d] for d in order], device=src.device,
                              dtype=out_dtype or src.dtype)
            out = out.permute([order.index(d) for d in range(len(shape))])
    sb = src if src.is_contiguous() else _Views.of_tensor(src, "src")
    db = out if out.is_contiguous() else _Views.of_tensor(out, "out")
    return sb, db, out, h, w, n


class CImageResizerParams(abi.Params):
    """avir::CImageResizerParams with the CImageResizerParamsDef values
    (avir.h:2262-2341); `preset` selects Def/ULR/LR/Low/High/Ultra."""
    PRESETS = {"def": 0, "ulr": 1, "lr": 2, "low": 3, "high": 4, "ultra": 5}

    def __init__(self, preset="def"):
        super().__init__()
        abi.load().avirhip_params_preset(self.PRESETS[preset], C.byref(self))


class CImageResizerVars(abi.Vars):
    """The caller-settable fields of avir::CImageResizerVars
    (avir.h:2516-2547): ox, oy, UseSRGBGamma, AlphaIndex, BuildMode, RndSeed."""

    def __init__(self):
        super().__init__()
        abi.load().avirhip_vars_default(C.byref(self))


class CImageResizer(object):
    """avir::CImageResizer<> (avir.h:4609): `CImageResizer(aResBitDepth=8,
    aSrcBitDepth=0, aParams=CImageResizerParamsDef())`. `aDitherer` stands
    for the reference's third fpclass_def template parameter (avir.h:4569):
    "def" = CImageResizerDithererDefINL, "errd" = CImageResizerDithererErrdINL
    (README.md:135-142); `aFpPack=4` stands for avir::fpclass_float4 of
    avir_float4_sse.h (README.md:174-186), `aFpPack=abi.FPCLASS_DOUBLE` for
    avir::fpclass_def<double> (avir.h:4553-4560: the double pipeline)."""

    DITHERERS = {"def": abi.DITHER_DEF, "errd": abi.DITHER_ERRD}

    def __init__(self, aResBitDepth=8, aSrcBitDepth=0, aParams=None,
                 aDitherer="def", aFpPack=1):
        self._lib = abi.load()
        self._h = C.c_void_p()
        abi.check(self._lib.avirhip_resizer_create(
            aResBitDepth, aSrcBitDepth,
            C.byref(aParams) if aParams is not None else None,
            C.byref(self._h)), "avirhip_resizer_create")
        if aDitherer != "def":
            abi.check(self._lib.avirhip_resizer_set_ditherer(
                self._h, self.DITHERERS[aDitherer]),
                "avirhip_resizer_set_ditherer")
        if aFpPack != 1:
            # fpclass_float4 of avir_float4_sse.h (fppack 4): its cost model,
            # nearest-even ditherer and float-output path
            abi.check(self._lib.avirhip_resizer_set_fpclass(self._h, aFpPack),
                      "avirhip_resizer_set_fpclass")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.avirhip_resizer_destroy(h)

    def resizeImage(self, SrcBuf, SrcWidth, SrcHeight, SrcScanlineSize, NewBuf,
                    NewWidth, NewHeight, ElCountIO, k, aVars=None):
        """resizeImage<Tin,Tout>() (avir.h:4680-4684). Tin/Tout are taken from
        the buffers' dtypes."""
        sp, sm, st, s1 = _buf(SrcBuf)
        dp, dm, dt, s2 = _buf(NewBuf)
        if SrcWidth > 0 and SrcHeight > 0 and NewWidth > 0 and NewHeight > 0:
            ss = SrcScanlineSize if SrcScanlineSize >= 1 else SrcWidth * ElCountIO
            _need(SrcBuf, (SrcHeight - 1) * ss + SrcWidth * ElCountIO, "SrcBuf")
            _need(NewBuf, NewWidth * NewHeight * ElCountIO, "NewBuf")
        elif NewWidth > 0 and NewHeight > 0:
            _need(NewBuf, NewWidth * NewHeight, "NewBuf")
        with _on_device_of(SrcBuf, NewBuf):
            abi.check(self._lib.avirhip_resizer_resize(
                self._h, sp, sm, SrcWidth, SrcHeight, SrcScanlineSize, dp, dm,
                NewWidth, NewHeight, ElCountIO, float(k),
                C.byref(aVars) if aVars is not None else None, st, dt,
                s1 or s2), "avirhip_resizer_resize")

    def plan(self, SrcWidth, SrcHeight, NewWidth, NewHeight, ElCountIO,
             k=0.0, aVars=None, in_type=F32, out_type=F32, SrcScanlineSize=0):
        """Returns the cached device plan handle (c_void_p) resizeImage()
        uses for this geometry -- for benchmarking and band execution."""
        p = C.c_void_p()
        abi.check(self._lib.avirhip_resizer_get_plan(
            self._h, SrcWidth, SrcHeight, SrcScanlineSize, NewWidth,
            NewHeight, ElCountIO, float(k),
            C.byref(aVars) if aVars is not None else None, in_type, out_type,
            C.byref(p)), "avirhip_resizer_get_plan")
        return p

    def band_source_rows(self, SrcWidth, SrcHeight, NewWidth, NewHeight,
                         ElCountIO, row0, row1, k=0.0, aVars=None,
                         in_type=F32, out_type=F32, SrcScanlineSize=0):
        """The source rows (first, last), inclusive, that output rows
        [row0, row1) read -- from the host planner alone, no GPU needed
        (avirhip_resizer_band_source_rows; SURVEY.md 8e: what a sharded frame's
        rank has to receive)."""
        a, b = C.c_int(), C.c_int()
        abi.check(self._lib.avirhip_resizer_band_source_rows(
            self._h, SrcWidth, SrcHeight, SrcScanlineSize, NewWidth, NewHeight,
            ElCountIO, float(k), C.byref(aVars) if aVars is not None else None,
            in_type, out_type, row0, row1, C.byref(a), C.byref(b)),
            "avirhip_resizer_band_source_rows")
        return a.value, b.value

    # Convenience (not part of the reference API).
    def resize(self, src, NewWidth, NewHeight, k=0.0, out_dtype=None,
               aVars=None):
        """src: (H, W, C) array/tensor -> new (NewHeight, NewWidth, C)."""
        h, w, ch = src.shape
        if _is_torch(src):
            import torch
            dst = torch.empty((NewHeight, NewWidth, ch), device=src.device,
                              dtype=out_dtype or src.dtype)
        else:
            dst = np.empty((NewHeight, NewWidth, ch), out_dtype or src.dtype)
        self.resizeImage(src, w, h, 0, dst, NewWidth, NewHeight, ch, k, aVars)
        return dst

    # Planes (an extension: the reference has no such call).
    def resizePlanes(self, SrcBuf, SrcWidth, SrcHeight, SrcScanlineSize,
                     NewBuf, NewWidth, NewHeight, PlaneCount, SrcPlaneSize=0,
                     NewPlaneSize=0, k=0.0, aVars=None):
        """`PlaneCount` single-channel planes of one geometry -- a
        channel-first image, a batch -- in one call
        (avirhip_resizer_resize_planes): plane i of the result is, bit for
        bit, resizeImage(..., ElCountIO=1, k, aVars) of plane i of the source.
        Planes lie `SrcPlaneSize` / `NewPlaneSize` elements apart (0: tightly
        packed); source rows at SrcScanlineSize, result rows tight. Either
        buffer may instead be a sequence of PlaneCount per-plane (H, W) CUDA
        tensors with any positive strides -- channel-last images, planes in
        separate allocations -- which go in as plane views (its plane size
        must then be 0)."""
        sp, sm, st, s1, sv = _plane_side(SrcBuf, SrcWidth, SrcHeight, "SrcBuf")
        dp, dm, dt, s2, dv = _plane_side(NewBuf, NewWidth, NewHeight, "NewBuf")
        for v in (sv, dv):
            if v is not None and v.count != PlaneCount:
                raise ValueError("resizePlanes: %d plane views, PlaneCount %d"
                                 % (v.count, PlaneCount))
        if sv is not None or dv is not None:
            pass    # (the library validates every view)
        elif min(SrcWidth, SrcHeight, NewWidth, NewHeight, PlaneCount) > 0:
            ss = SrcScanlineSize if SrcScanlineSize >= 1 else SrcWidth
            sps = SrcPlaneSize if SrcPlaneSize != 0 else SrcHeight * ss
            nps = NewPlaneSize if NewPlaneSize != 0 else NewHeight * NewWidth
            _need(SrcBuf, (PlaneCount - 1) * sps + (SrcHeight - 1) * ss
                  + SrcWidth, "SrcBuf")
            _need(NewBuf, (PlaneCount - 1) * nps + NewHeight * NewWidth,
                  "NewBuf")
        elif min(NewWidth, NewHeight, PlaneCount) > 0:
            nps = NewPlaneSize if NewPlaneSize != 0 else NewHeight * NewWidth
            _need(NewBuf, (PlaneCount - 1) * nps + NewHeight * NewWidth,
                  "NewBuf")
        with _on_device_of(_device_of(SrcBuf), _device_of(NewBuf)):
            abi.check(self._lib.avirhip_resizer_resize_planes(
                self._h, sp, sm, SrcWidth, SrcHeight, SrcScanlineSize, dp, dm,
                NewWidth, NewHeight, PlaneCount, SrcPlaneSize, NewPlaneSize,
                float(k), C.byref(aVars) if aVars is not None else None, st,
                dt, s1 or s2), "avirhip_resizer_resize_planes")

    def resize_planes(self, src, NewWidth, NewHeight, k=0.0, out_dtype=None,
                      aVars=None, out=None):
        """src: a (..., H, W) array/tensor -> new (..., NewHeight, NewWidth);
        all leading dimensions fold into the plane count. A CUDA tensor need
        not be contiguous (channels_last, x.permute(0, 3, 1, 2) of an NHWC
        tensor, slices: any positive strides): it is read where it lies, as
        plane views, and the result keeps its memory format. `out`: the result
        tensor, with the same freedom."""
        sb, db, dst, h, w, n = _planes_operands(src, NewWidth, NewHeight,
                                                out_dtype, out)
        self.resizePlanes(sb, w, h, 0, db, NewWidth, NewHeight, n, 0, 0, k,
                          aVars)
        return dst


class CLancIRParams(abi.LancirParams):
    """avir::CLancIRParams (lancir.h:260-307)."""

    def __init__(self, aSrcSSize=0, aNewSSize=0, akx=0.0, aky=0.0, aox=0.0,
                 aoy=0.0):
        super().__init__()
        self.SrcSSize, self.NewSSize = aSrcSSize, aNewSSize
        self.kx, self.ky, self.ox, self.oy, self.la = akx, aky, aox, aoy, 3.0


class CLancIR(object):
    """avir::CLancIR (lancir.h:327)."""

    def __init__(self):
        self._lib = abi.load()
        self._h = C.c_void_p()
        abi.check(self._lib.avirhip_lancir_create(C.byref(self._h)),
                  "avirhip_lancir_create")

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.avirhip_lancir_destroy(h)

    def resizeImage(self, SrcBuf, SrcWidth, SrcHeight, NewBuf, NewWidth,
                    NewHeight, ElCount, aParams=None):
        """resizeImage<Tin,Tout>() (lancir.h:386-390): returns NewHeight, or
        0 on a parameter error."""
        if SrcBuf is None or NewBuf is None:
            return 0
        sp, sm, st, s1 = _buf(SrcBuf)
        dp, dm, dt, s2 = _buf(NewBuf)
        if (min(SrcWidth, SrcHeight, NewWidth, NewHeight, ElCount) > 0
                and sp != dp):  # SrcBuf == NewBuf is the library's error 0
            ss = aParams.SrcSSize if aParams is not None else 0
            ns = aParams.NewSSize if aParams is not None else 0
            ss = ss if ss >= 1 else SrcWidth * ElCount
            ns = ns if ns >= 1 else NewWidth * ElCount
            _need(SrcBuf, (SrcHeight - 1) * ss + SrcWidth * ElCount, "SrcBuf")
            _need(NewBuf, (NewHeight - 1) * ns + NewWidth * ElCount, "NewBuf")
        with _on_device_of(SrcBuf, NewBuf):
            rc = self._lib.avirhip_lancir_resize(
                self._h, sp, sm, SrcWidth, SrcHeight, dp, dm, NewWidth,
                NewHeight, ElCount,
                C.byref(aParams) if aParams is not None else None, st, dt,
                s1 or s2)
        return abi.check(rc, "avirhip_lancir_resize")

    def plan(self, SrcWidth, SrcHeight, NewWidth, NewHeight, ElCount,
             aParams=None, in_type=F32, out_type=F32):
        p = C.c_void_p()
        abi.check(self._lib.avirhip_lancir_get_plan(
            self._h, SrcWidth, SrcHeight, NewWidth, NewHeight, ElCount,
            C.byref(aParams) if aParams is not None else None, in_type,
            out_type, C.byref(p)), "avirhip_lancir_get_plan")
        return p

    def band_source_rows(self, SrcWidth, SrcHeight, NewWidth, NewHeight,
                         ElCount, row0, row1, aParams=None, in_type=F32,
                         out_type=F32):
        """(first, last) source rows of output rows [row0, row1); host only."""
        a, b = C.c_int(), C.c_int()
        abi.check(self._lib.avirhip_lancir_band_source_rows(
            self._h, SrcWidth, SrcHeight, NewWidth, NewHeight, ElCount,
            C.byref(aParams) if aParams is not None else None, in_type,
            out_type, row0, row1, C.byref(a), C.byref(b)),
            "avirhip_lancir_band_source_rows")
        return a.value, b.value

    def resize(self, src, NewWidth, NewHeight, out_dtype=None, aParams=None):
        h, w, ch = src.shape
        if _is_torch(src):
            import torch
            dst = torch.empty((NewHeight, NewWidth, ch), device=src.device,
                              dtype=out_dtype or src.dtype)
        else:
            dst = np.empty((NewHeight, NewWidth, ch), out_dtype or src.dtype)
        rc = self.resizeImage(src, w, h, dst, NewWidth, NewHeight, ch, aParams)
        if rc != NewHeight:
            raise AvirHipError("CLancIR.resizeImage returned %d" % rc)
        return dst

    # Planes (an extension: the reference has no such call).
    def resizePlanes(self, SrcBuf, SrcWidth, SrcHeight, NewBuf, NewWidth,
                     NewHeight, PlaneCount, SrcPlaneSize=0, NewPlaneSize=0,
                     aParams=None):
        """`PlaneCount` single-channel planes of one geometry -- a
        channel-first image, a batch -- in one call
        (avirhip_lancir_resize_planes): plane i of the result is, bit for
        bit, resizeImage(..., ElCount=1) of plane i of the source. Planes lie
        `SrcPlaneSize` / `NewPlaneSize` elements apart (0: tightly packed);
        rows at aParams.SrcSSize / NewSSize. Either buffer may instead be a
        sequence of PlaneCount per-plane (H, W) CUDA tensors with any positive
        strides, which go in as plane views (its plane size must then be 0).
        Returns NewHeight, or 0 on a parameter error."""
        if SrcBuf is None or NewBuf is None:
            return 0
        sp, sm, st, s1, sv = _plane_side(SrcBuf, SrcWidth, SrcHeight, "SrcBuf")
        dp, dm, dt, s2, dv = _plane_side(NewBuf, NewWidth, NewHeight, "NewBuf")
        for v in (sv, dv):
            if v is not None and v.count != PlaneCount:
                raise ValueError("resizePlanes: %d plane views, PlaneCount %d"
                                 % (v.count, PlaneCount))
        if sv is not None or dv is not None:
            pass    # (the library validates every view)
        elif (min(SrcWidth, SrcHeight, NewWidth, NewHeight, PlaneCount) > 0
                and sp != dp):
            ss = aParams.SrcSSize if aParams is not None else 0
            ns = aParams.NewSSize if aParams is not None else 0
            ss = ss if ss >= 1 else SrcWidth
            ns = ns if ns >= 1 else NewWidth
            sps = SrcPlaneSize if SrcPlaneSize != 0 else SrcHeight * ss
            nps = NewPlaneSize if NewPlaneSize != 0 else NewHeight * ns
            _need(SrcBuf, (PlaneCount - 1) * sps + (SrcHeight - 1) * ss
                  + SrcWidth, "SrcBuf")
            _need(NewBuf, (PlaneCount - 1) * nps + (NewHeight - 1) * ns
                  + NewWidth, "NewBuf")
        with _on_device_of(_device_of(SrcBuf), _device_of(NewBuf)):
            rc = self._lib.avirhip_lancir_resize_planes(
                self._h, sp, sm, SrcWidth, SrcHeight, dp, dm, NewWidth,
                NewHeight, PlaneCount, SrcPlaneSize, NewPlaneSize,
                C.byref(aParams) if aParams is not None else None, st, dt,
                s1 or s2)
        return abi.check(rc, "avirhip_lancir_resize_planes")

    def resize_planes(self, src, NewWidth, NewHeight, out_dtype=None,
                      aParams=None, out=None):
        """src: a (..., H, W) array/tensor -> new (..., NewHeight, NewWidth);
        all leading dimensions fold into the plane count. A CUDA tensor need
        not be contiguous (channels_last, permuted NHWC, slices: any positive
        strides): it is read where it lies, as plane views, and the result
        keeps its memory format. `out`: the result tensor, with the same
        freedom."""
        sb, db, dst, h, w, n = _planes_operands(src, NewWidth, NewHeight,
                                                out_dtype, out)
        rc = self.resizePlanes(sb, w, h, db, NewWidth, NewHeight, n, 0, 0,
                               aParams)
        if rc != NewHeight:
            raise AvirHipError("CLancIR.resizePlanes returned %d" % rc)
        return dst
