"""Decoded images as torch tensors on the GPU that decoded them: a Pipeline batch into scratch canvases, then ONE jda_pack_surfaces launch
straight into the tensors' memory (include/jpegdec_amd.h: dense RGB / BGR or planar CHW, uint8 or float through a lookup table).  With
size=(H, W) ONE jda_resize_surfaces launch (Pillow's antialiased BILINEAR, bit for bit) stands between the two, and the result is one batch.
encode_tensors is the way back: ONE jda_unpack_surfaces launch from the tensors' own memory into scratch surfaces, one encode call, JPEG files out.
torch is imported when decode_to_tensors or encode_tensors runs, not when the package is.  One process, one HIP runtime: a torch build that ships its own
(a wheel does) must be imported BEFORE libjpegdec_amd.so is loaded (before the first Context), so that the library binds to the runtime
torch already brought; the other way round the process holds two runtimes, torch finds no GPU, and decode_to_tensors says so."""
import ctypes as C

import numpy as np

from . import binding as B


def _np_dtype(dtype):
    """numpy's float16 / float32 / uint8 for a numpy or torch dtype (or their names)"""
    name = str(dtype).replace("torch.", "").replace("<class 'numpy.", "").replace("'>", "")
    try:
        return {"uint8": np.uint8, "float16": np.float16, "half": np.float16, "float32": np.float32, "float": np.float32}[name]
    except KeyError:
        raise ValueError("no packed element type for dtype %r: uint8, float16 or float32" % (dtype,))


def normalise_table(mean, std, dtype=np.float32):
    """The lookup table of the usual input normalisation: table[c][v] = (v / 255 - mean[c]) / std[c], worked out in float64 and cast to
    dtype (float16 or float32) -- a numpy array [len(mean), 256] for pack_surfaces / decode_packed_to_host / decode_to_tensors.  The channel
    is the DESTINATION channel: with BGR output, mean[0] is blue's."""
    mean, std = np.atleast_1d(np.asarray(mean, np.float64)), np.atleast_1d(np.asarray(std, np.float64))
    if mean.shape != std.shape or mean.ndim != 1:
        raise ValueError("mean and std: one value per channel each")
    t = (np.arange(256, dtype=np.float64)[None, :] / 255.0 - mean[:, None]) / std[:, None]
    return np.ascontiguousarray(t.astype(_np_dtype(dtype)))


def denormalise_params(mean, std):
    """The inverse of normalise_table for unpack_surfaces / encode_dense_to_host / encode_tensors: a float32 array [2, C] = (scale, bias) with
    scale[c] = 255 * std[c], bias[c] = 255 * mean[c], worked out in float64 and cast to float32 -- a tensor normalised as (v / 255 - mean) /
    std becomes bytes again as clamp(rint(x * scale + bias), 0, 255).  The channel is the TENSOR channel: with BGR tensors, mean[0] is blue's."""
    mean, std = np.atleast_1d(np.asarray(mean, np.float64)), np.atleast_1d(np.asarray(std, np.float64))
    if mean.shape != std.shape or mean.ndim != 1:
        raise ValueError("mean and std: one value per channel each")
    return np.ascontiguousarray(np.stack([255.0 * std, 255.0 * mean]).astype(np.float32))


def encode_tensors(ctx, images, quality=75, sampling="4:2:0", restart_interval=0, optimize=False, progressive=False, layout="CHW", bgr=False, scale_bias=None):
    """images -> list of JPEG files (bytes).  images: ONE [N,C,H,W] / [N,H,W,C] tensor, or a list of [C,H,W] / [H,W,C] tensors of any sizes
    (layout "CHW" or "HWC"; bgr: channel 0 is blue) -- all on cuda:<ctx.device>, all of one dtype (torch.uint8, float16 or float32), all of
    one C (3, or 1: gray, which takes the gray sampling whatever `sampling` says); anything else is a ValueError before the GPU is touched.
    uint8: the bytes themselves.  float: byte = clamp(rint(x * scale[c] + bias[c]), 0, 255), scale_bias = (scale[C], bias[C]) -- None: (255,
    0), for values in [0, 1]; denormalise_params(mean, std) for a normalised tensor.  optimize / progressive / restart_interval: as
    thumbnails().  One jda_unpack_surfaces launch from the tensors' own memory into scratch surfaces, one encode call; only the files are
    copied back.  The tensors must be complete on torch's side: the call synchronises the device before its first launch."""
    import torch

    if layout not in ("CHW", "HWC"):
        raise ValueError("layout: 'CHW' or 'HWC'")
    if isinstance(images, torch.Tensor):
        if images.dim() != 4:
            raise ValueError("images: one [N,C,H,W] / [N,H,W,C] tensor, or a list of [C,H,W] / [H,W,C] tensors")
        images = [images[k] for k in range(images.shape[0])]
    else:
        images = list(images)
        if any(not isinstance(t, torch.Tensor) or t.dim() != 3 for t in images):
            raise ValueError("images: one [N,C,H,W] / [N,H,W,C] tensor, or a list of [C,H,W] / [H,W,C] tensors")
    n = len(images)
    if n == 0:
        return []
    device = torch.device("cuda", ctx.device)
    if any(t.device != device for t in images):
        raise ValueError("images: all on %s" % device)
    if any(t.dtype != images[0].dtype for t in images):
        raise ValueError("images: all of one dtype")
    npdt = _np_dtype(images[0].dtype)
    elem = {np.uint8: B.PACK_U8, np.float16: B.PACK_F16, np.float32: B.PACK_F32}[npdt]
    dims = [(t.shape[0], t.shape[1], t.shape[2]) if layout == "CHW" else (t.shape[2], t.shape[0], t.shape[1]) for t in images]      # (C, H, W)
    channels = dims[0][0]
    if channels not in (1, 3) or any(d[0] != channels for d in dims):
        raise ValueError("images: all of 3 channels or all of 1")
    if any(d[1] <= 0 or d[2] <= 0 for d in dims):
        raise ValueError("images: empty")
    if bgr and channels == 1:
        raise ValueError("bgr: not with one channel")
    if elem == B.PACK_U8 and scale_bias is not None:
        raise ValueError("scale_bias: with float16 / float32 tensors")
    if scale_bias is not None:
        scale_bias = np.asarray(scale_bias.detach().cpu().numpy() if isinstance(scale_bias, torch.Tensor) else scale_bias, np.float32).reshape(-1)
        if scale_bias.size != 2 * channels or not np.all(np.isfinite(scale_bias)):
            raise ValueError("scale_bias: %d finite scales and %d finite biases" % (channels, channels))
    if progressive and restart_interval != 0:
        raise ValueError("progressive: restart_interval must be 0")
    bpp = 4 if channels == 3 else 1
    if isinstance(sampling, str) and sampling not in B.ENCODE_SAMPLINGS:
        raise ValueError("sampling: one of %s" % ", ".join(repr(k) for k in B.ENCODE_SAMPLINGS))
    samp = B.ENCODE_GRAY if channels == 1 else B.ENCODE_SAMPLINGS[sampling] if isinstance(sampling, str) else int(sampling)
    flags = (B.PACK_CHW if layout == "CHW" else B.PACK_HWC) | (B.PACK_BGR if bgr else 0)
    dense = [t.contiguous() for t in images]                              # (the copies live until this function returns: behind the encode call)
    pitches = [(w * bpp + 15) & ~15 for _, h, w in dims]
    caps = [B.encode_bound_progressive(w, h, samp) if progressive else B.encode_bound(w, h, samp, restart_interval) for _, h, w in dims]
    soffs, total = [], 0
    for p, (_, h, w) in zip(pitches, dims):
        soffs.append(total)
        total += (p * h + 255) & ~255
    foffs = []
    for c in caps:
        foffs.append(total)
        total += (c + 255) & ~255
    torch.cuda.synchronize(device)                                        # (the tensors were written on torch's stream)
    base = ctx.malloc(total)
    try:
        surfaces = [(base + soffs[k], pitches[k], dims[k][2], dims[k][1]) for k in range(n)]
        B.unpack_surfaces(ctx, [t.data_ptr() for t in dense], surfaces, bpp, flags, elem, scale_bias)
        jobs, dsts = [(0, 0, dims[k][2], dims[k][1], samp, quality, restart_interval) for k in range(n)], [base + foffs[k] for k in range(n)]
        if progressive:
            nbytes, st = B.encode_surfaces_progressive(ctx, surfaces, bpp, jobs, dsts, caps)
        else:
            nbytes, st = B.encode_surfaces(ctx, surfaces, bpp, jobs, dsts, caps, [B.ENCODE_OPTIMIZE] * n if optimize else None)
        if any(st):
            raise B.JdaError(max(st), "jda_encode_surfaces")
        # (the files alone come back: nbytes[k] bytes each)
        return [ctx.to_host(base + foffs[k], nbytes[k]).tobytes() for k in range(n)]
    finally:
        ctx.free(base)


def prescale_option(info, pixel_type, options, size):
    """The largest of SCALE_HALF / QUARTER / EIGHTH with which the file's visible size is still at least size = (H, W) on both axes, or 0"""
    for bit in (B.SCALE_EIGHTH, B.SCALE_QUARTER, B.SCALE_HALF):
        g = B.output_geometry(info, pixel_type, options | bit)
        if g["out_w"] >= size[1] and g["out_h"] >= size[0]:
            return bit
    return 0


def _exact_batch(ctx, files, infos, outs, pt, scales=None, colour_models=False, rects=None):
    """decode_to_tensors(decoder="libjpeg"): the files resident -- baseline ones with the device pre-scan's index, progressive ones as
    coefficient images in whichever form is smaller -- and ONE exact_decode call into the surfaces `outs` (scales: file k at 1 / scales[k],
    libjpeg's scaled decode; colour_models: exact_decode's; rects: exact_decode's -- the surfaces then hold the rectangles); -> the statuses"""
    n = len(files)
    # (CMYK, YCCK, and an extended-sequential frame, which jda_prepare does not take: a coefficient image whatever the SOF type)
    four = [colour_models and (infos[k].ncomp == 4 or getattr(infos[k], "via_coef_prepare", False)) for k in range(n)]
    base_ix = [k for k in range(n) if infos[k].jpeg_type != 1 and not four[k]]
    prepared, sources, hosts = [], [None] * n, []
    try:
        prepared = B.prepare_batch([files[k] for k in base_ix], device_prescan=True) if base_ix else []
        for k, d in zip(base_ix, B.upload_batch(ctx, prepared) if base_ix else []):
            sources[k] = d
        for k in range(n):
            if infos[k].jpeg_type == 1 or four[k]:
                hosts.append(B.CoefImage.from_file(files[k]) if four[k] else B.CoefImage(files[k]))
                sources[k] = B.DeviceCoef(ctx, hosts[-1], B.COEF_AUTO)
        return B.exact_decode(ctx, sources, outs, [pt] * n, scales, colour_models, rects)
    finally:
        for d in sources:
            if d is not None:
                d.close()
        for p in list(prepared) + hosts:
            if p is not None:
                p.close()


def decode_to_tensors(ctx, files, layout="CHW", dtype=None, table=None, options=0, bgr=False, size=None, crops=None, prescale=False, progressive="thumbnail", resample=None,
                      decoder="reference", draft=None, colour_models=False):
    """files (JPEG bytes, all colour or all gray) -> tensors on cuda:<ctx.device>.  layout "CHW" or "HWC"; dtype torch.uint8 (default), or
    torch.float16 / torch.float32 with table = [C, 256] values of that type (normalise_table; numpy or torch).  options: the decode option
    bits of every file (a JDA_SCALE_* bit, JDA_LUMA_ONLY: one channel).  Returns a list of [C,H,W] / [H,W,C] tensors, or, when all images
    have one size, ONE [N,C,H,W] / [N,H,W,C] tensor.  A file that fails to decode raises JdaError with its status.
    size = (H, W): every image -- or crops[k] = (x, y, w, h) of image k, in pixels of its visible size -- is resized to H x W on the GPU
    (jda_resize_surfaces_ex: Pillow's resize(F, box), bit for bit) before it is packed, and the result is always ONE [N,C,H,W] /
    [N,H,W,C] tensor.  resample: F -- "bilinear" (the default), "box", "hamming", "bicubic" or "lanczos", or the id (RESIZE_*); it goes
    with size=.  prescale=True (whole images only): each file is decoded at the largest of 1/2, 1/4, 1/8 whose visible size is still
    at least W x H on both axes -- the DCT-domain shortcut for thumbnails; it changes pixels, so it is opt-in.
    progressive="thumbnail" (the default): a progressive file comes back as the reference decodes it, the 1/8 thumbnail of its first scan.
    progressive="full": every file whose header says progressive gets PROGRESSIVE_FULL in its options and the batch is submitted with
    SUBMIT_PROGRESSIVE_FULL -- every scan, full size, so a batch that mixes baseline and progressive files of one size is still ONE
    tensor; size= and crops= work as for any file.  There is no DCT-domain scale for such a file: with prescale=True it is decoded at full
    size and resized from there, and a JDA_SCALE_* bit in options is refused for it (JdaError 3).
    decoder="reference" (the default): the decode stages that reproduce the reference decoder, through a Pipeline batch.  decoder="libjpeg":
    libjpeg's own arithmetic (jda_exact_decode_surfaces: islow IDCT, fancy upsampling, 16-bit colour constants), so that the pixels in
    front of the resize are Image.open(f).convert("RGB")'s and, with size= and resample=, the tensor is Pillow's resize() of them bit for
    bit.  Baseline files go through prepare_batch(device_prescan=True) + upload_batch, progressive ones -- every scan, whatever
    progressive= says -- through CoefImage + jda_coef_upload_ex(COEF_AUTO), then ONE exact_decode call into the scratch surfaces.  The
    reference road's scales are not libjpeg's: prescale=True or a JDA_SCALE_* bit in options is a ValueError (libjpeg's own reduced-size
    decode is draft=, below), and so is every other option bit but
    JDA_LUMA_ONLY (one channel: the Y plane, Pillow's draft("L")) -- none is silently dropped.
    draft (decoder="libjpeg" with size=, whole images): Pillow's Image.draft() in front of the resize.  draft=True requests `size` itself,
    draft=(h, w) any other size; each file is decoded at the scale Pillow would choose for that request (exact_draft_scale: the largest of
    1/8, 1/4, 1/2, 1 that keeps both sides at or above it) by libjpeg's reduced-size IDCTs (jda_exact_decode_surfaces_scaled) and resized
    from there, so that the tensor is Pillow's draft() -> convert("RGB") -> resize() bit for bit.  With decoder="reference", with crops= or
    without size= it is a ValueError.  With crops= this road decodes of each file only the MCUs the resize of its crop reads
    (jda_exact_decode_surfaces_rect, into a surface of that rectangle's size); the tensor is the one a whole decode gives.
    colour_models (decoder="libjpeg"; jda_exact_decode_surfaces_ex with JDA_EXACT_COLOUR_MODELS): True takes files with an Adobe APP14 segment
    and reads every one- or three-component file by libjpeg's own rule (exact_probe) -- Photoshop's YCbCr files (transform 1) as any YCbCr
    file, RGB-coded ones (Adobe transform 0 without JFIF, or component ids 'R', 'G', 'B' without either marker) as the R, G, B they hold.
    Without it such files are refused (JdaError 3) or, the RGB-coded ones without a segment, converted as if they were YCbCr.  Four-component
    files (CMYK, YCCK; baseline or progressive) go through CoefImage.from_file and come out as Pillow's convert("RGB") of them; draft= leaves
    them at full size only where Pillow's scale would be 1 (a reduced-size decode of four components is JdaError 3).  With
    decoder="reference" it is a ValueError."""
    files = list(files)
    if decoder not in ("reference", "libjpeg"):
        raise ValueError("decoder: 'reference' or 'libjpeg'")
    if draft is not None and draft is not False:
        if decoder != "libjpeg" or size is None or crops is not None:
            raise ValueError("draft goes with decoder='libjpeg' and size=(H, W), whole images only")
        if draft is not True:
            draft = tuple(int(v) for v in draft)
            if len(draft) != 2 or draft[0] <= 0 or draft[1] <= 0:
                raise ValueError("draft: True or (h, w), both positive")
    else:
        draft = None
    if decoder == "libjpeg" and (prescale or options & (B.SCALE_HALF | B.SCALE_QUARTER | B.SCALE_EIGHTH)):
        raise ValueError("decoder='libjpeg': no prescale, no JDA_SCALE_* bit in options (the reference road's scales); libjpeg's scaled decode is draft=")
    if decoder == "libjpeg" and options & ~B.LUMA_ONLY:
        raise ValueError("decoder='libjpeg': the only option bit it honours is JDA_LUMA_ONLY (the Y plane)")
    if colour_models and decoder != "libjpeg":
        raise ValueError("colour_models goes with decoder='libjpeg'")
    if progressive not in ("thumbnail", "full"):
        raise ValueError("progressive: 'thumbnail' or 'full'")
    if layout not in ("CHW", "HWC"):
        raise ValueError("layout: 'CHW' or 'HWC'")
    if size is None:
        if crops is not None or prescale or resample is not None:
            raise ValueError("crops, prescale and resample go with size=(H, W)")
    else:
        filt = B.resize_filter("bilinear" if resample is None else resample)
        size = tuple(int(v) for v in size)
        if len(size) != 2 or size[0] <= 0 or size[1] <= 0:
            raise ValueError("size: (H, W), both positive")
        if crops is not None and prescale:
            raise ValueError("prescale is for whole images: not with crops")
        if prescale and options & (B.SCALE_HALF | B.SCALE_QUARTER | B.SCALE_EIGHTH):
            raise ValueError("prescale chooses the scale: no JDA_SCALE_* bit in options")
        if crops is not None:
            crops = [tuple(int(v) for v in c) for c in crops]
            if len(crops) != len(files) or any(len(c) != 4 for c in crops):
                raise ValueError("crops: one (x, y, w, h) per file")
    import torch

    if not torch.cuda.is_available():
        raise RuntimeError("torch sees no GPU in this process: if libjpegdec_amd.so was loaded first (a Context exists) and torch ships a HIP "
                           "runtime of its own, the process holds two runtimes -- import torch before the first jpegdec_amd.Context")
    dtype = torch.uint8 if dtype is None else dtype
    npdt = _np_dtype(dtype)
    elem = {np.uint8: B.PACK_U8, np.float16: B.PACK_F16, np.float32: B.PACK_F32}[npdt]
    es = np.dtype(npdt).itemsize
    flags = (B.PACK_CHW if layout == "CHW" else B.PACK_HWC) | (B.PACK_BGR if bgr else 0)
    n = len(files)
    device = torch.device("cuda", ctx.device)
    if n == 0:
        return []
    infos = []
    for f in files:
        info = B.ImageInfo()
        rc = ctx.lib.jda_parse(f, len(f), C.byref(info))
        if rc == 3 and colour_models:                                    # (an SOF1 frame, perhaps: jda_coef_prepare reads those, and keeps the header)
            host = B.CoefImage.from_file(f)
            info = B.ImageInfo.from_buffer_copy(host.info)
            info.via_coef_prepare = True
            host.close()
        elif rc != 0:
            raise B.JdaError(rc, "jda_parse")
        infos.append(info)
    gray = [i.ncomp == 1 or bool(options & B.LUMA_ONLY) for i in infos]
    if any(gray) != all(gray) and not (colour_models and not options & B.LUMA_ONLY):
        raise ValueError("gray and colour files in one call: one jda_pack_surfaces launch takes one source format")
    # (colour_models: a gray file among colour ones comes out as Pillow's convert("RGB") of it, R = G = B = Y)
    pt, channels = (B.GRAY8, 1) if all(gray) else (B.RGB8888, 3)
    full = [(progressive == "full" or decoder == "libjpeg") and i.jpeg_type == 1 for i in infos]
    opts = [options | B.PROGRESSIVE_FULL if fl else options | (prescale_option(i, pt, options, size) if prescale else 0) for i, fl in zip(infos, full)]
    geos = [B.output_geometry(i, pt, o) for i, o in zip(infos, opts)]
    scales = None
    if draft is not None:                                               # (the surfaces are then the scaled images, nothing around them)
        req = size if draft is True else draft
        scales = [B.exact_draft_scale(i, (req[1], req[0])) for i in infos]
        for k, (i, s) in enumerate(zip(infos, scales)):
            w, h = -(-i.width // s), -(-i.height // s)
            geos[k] = dict(geos[k], canvas_w=w, canvas_h=h, out_w=w, out_h=h)
    rects = None
    if decoder == "libjpeg" and crops is not None:
        # only what the resize reads of each file is decoded (jda_exact_decode_surfaces_rect): the source rectangle of the filter's taps for
        # the crop, clipped at the image, into a surface of that size; the crop moves by the rectangle's origin.  (A four-component file has
        # no rectangle decode: it stays whole.)
        rects, crops = [None] * n, list(crops)
        for k, i in enumerate(infos):
            if i.ncomp == 4:
                continue
            x0, y0, x1, y1 = B.resize_reads((i.width, i.height), crops[k], (size[1], size[0]), filt)
            rects[k] = (x0, y0, x1 - x0, y1 - y0)
            crops[k] = (crops[k][0] - x0, crops[k][1] - y0, crops[k][2], crops[k][3])
            geos[k] = dict(geos[k], canvas_w=x1 - x0, canvas_h=y1 - y0, out_w=x1 - x0, out_h=y1 - y0)
    bpp = 4 if (decoder == "libjpeg" and pt == B.RGB8888) else geos[0]["bpp"]
    pitches = [(g["canvas_w"] * bpp + 15) & ~15 for g in geos]
    offs, total = [], 0
    for g, p in zip(geos, pitches):
        offs.append(total)
        total += (p * g["canvas_h"] + 255) & ~255
    sizes = [(g["out_h"], g["out_w"]) if size is None else size for g in geos]
    same = all(s == sizes[0] for s in sizes)
    # size=(H, W): a second scratch allocation of H x W surfaces behind the canvases, the resize launch's destinations and the pack launch's sources
    rpitch = 0 if size is None else (size[1] * bpp + 15) & ~15
    rbytes = 0 if size is None else (rpitch * size[0] + 255) & ~255

    def shape(h, w):
        return (channels, h, w) if layout == "CHW" else (h, w, channels)
    if same:
        whole = torch.empty((n,) + shape(*sizes[0]), dtype=dtype, device=device)
        per = whole[0].numel() * es
        ptrs = [whole.data_ptr() + k * per for k in range(n)]          # (image k at its own, unaligned, offset)
        result = whole
    else:
        result = [torch.empty(shape(h, w), dtype=dtype, device=device) for h, w in sizes]
        ptrs = [t.data_ptr() for t in result]
    dev_table = None
    if table is not None:
        host = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
        if host.dtype != npdt or host.size != channels * 256:
            raise ValueError("table: %d x 256 values of %s" % (channels, np.dtype(npdt).name))
        dev_table = torch.from_numpy(np.ascontiguousarray(host).reshape(channels, 256)).to(device)
        torch.cuda.synchronize(device)                                   # (the table's copy ran on torch's stream)
    base = ctx.malloc(total)
    rbase = None
    try:
        if size is not None:
            rbase = ctx.malloc(rbytes * n)
        outs = [(base + offs[k], pitches[k], geos[k]["canvas_w"], geos[k]["canvas_h"]) for k in range(n)]
        if decoder == "libjpeg":
            status = _exact_batch(ctx, files, infos, outs, pt, scales, bool(colour_models), rects)
        else:
            pipe = B.Pipeline(ctx, max_images=n, depth=1)
            try:
                status = pipe.wait(pipe.submit(files, outs, [pt] * n, opts, B.SUBMIT_PROGRESSIVE_FULL if any(full) else 0))
            finally:
                pipe.close()
        for k, st in enumerate(status):
            if st != 0:
                raise B.JdaError(st, "file %d of the batch" % k)
        # the VISIBLE rectangles of the canvases, one launch, straight into the tensors -- or resized first, where they lie, in one launch
        visible = [(base + offs[k], pitches[k], geos[k]["out_w"], geos[k]["out_h"]) for k in range(n)]
        if size is not None:
            resized = [(rbase + k * rbytes, rpitch, size[1], size[0]) for k in range(n)]
            B.resize_surfaces(ctx, visible, bpp, resized, crops, filt)
            visible = resized
        B.pack_surfaces(ctx, visible, bpp, ptrs, flags, elem, None if dev_table is None else dev_table.data_ptr())
    finally:
        ctx.free(base)
        if rbase is not None:
            ctx.free(rbase)
    return result


def _libjpeg_table_order(f):
    """The Huffman table segments in front of a file's first scan in the order libjpeg writes them: per component of the scan its DC table,
    then its AC table -- DC 0, AC 0, DC 1, AC 1.  jda_encode_surfaces writes a standard-table colour file's four segments as DC 0, DC 1,
    AC 0, AC 1 (the same segments; every decoder reads either order, and its contract is the bytes behind the SOS header): a file that has
    to be Pillow's from the first byte to the last gets them moved here, on the host, in the few hundred bytes of its header.  A file whose
    segments already stand in that order (gray, optimised and progressive files) comes back as it is."""
    i, first, end, segs = 2, None, 0, []
    while i + 4 <= len(f) and f[i] == 0xFF and f[i + 1] != 0xDA:
        length = (f[i + 2] << 8) | f[i + 3]
        if f[i + 1] == 0xC4:
            first = i if first is None else first
            segs.append(f[i:i + 2 + length])
            end = i + 2 + length
        elif first is not None:
            break
        i += 2 + length
    if first is None:
        return f
    return f[:first] + b"".join(sorted(segs, key=lambda s: (s[4] & 15, s[4] >> 4))) + f[end:]


def _pillow_thumbnails(ctx, files, infos, size, filt, gap, pt, samp, quality, restart_interval, optimize, progressive):
    """thumbnails(pillow=True): the plans, ONE exact decode at the plans' scales, one reduce launch over the files that have that step, one
    float-box resize launch over those that are resized, one encode call over every file's final surface"""
    n = len(files)
    plans = [B.thumbnail_plan(i.width, i.height, size, filt, gap) for i in infos]       # (JdaError for a plan the call cannot run)
    bpp = 1 if pt == B.GRAY8 else 4
    total = 0

    def surface(w, h):
        nonlocal total
        pitch = (w * bpp + 15) & ~15
        at = total
        total += (pitch * h + 255) & ~255
        return [at, pitch, w, h]

    draft = [surface(*p["draft"]) for p in plans]
    reduced = [surface(*p["reduced"]) if p["factors"] != (1, 1) else None for p in plans]
    final = [surface(*p["out"]) if p["resize"] else None for p in plans]
    caps, foffs = [], []
    for p in plans:
        caps.append(B.encode_bound_progressive(p["out"][0], p["out"][1], samp) if progressive else B.encode_bound(p["out"][0], p["out"][1], samp, restart_interval))
        foffs.append(total)
        total += (caps[-1] + 255) & ~255
    base = ctx.malloc(total)
    try:
        at = lambda q: (base + q[0], q[1], q[2], q[3])
        status = _exact_batch(ctx, files, infos, [at(q) for q in draft], pt, [p["scale"] for p in plans])
        for k, st in enumerate(status):
            if st != 0:
                raise B.JdaError(st, "file %d of the batch" % k)
        cur = list(draft)
        ks = [k for k in range(n) if reduced[k] is not None]
        if ks:
            B.reduce_surfaces(ctx, [at(cur[k]) for k in ks], bpp, [plans[k]["factors"] for k in ks], [at(reduced[k]) for k in ks], [plans[k]["reduce_box"] for k in ks])
            for k in ks:
                cur[k] = reduced[k]
        ks = [k for k in range(n) if final[k] is not None]
        if ks:
            B.resize_surfaces_box(ctx, [at(cur[k]) for k in ks], bpp, [at(final[k]) for k in ks], [plans[k]["box"] for k in ks], filt)
            for k in ks:
                cur[k] = final[k]
        jobs = [(0, 0, p["out"][0], p["out"][1], samp, quality, restart_interval) for p in plans]
        dsts = [base + o for o in foffs]
        if progressive:
            nbytes, st = B.encode_surfaces_progressive(ctx, [at(q) for q in cur], bpp, jobs, dsts, caps)
        else:
            nbytes, st = B.encode_surfaces(ctx, [at(q) for q in cur], bpp, jobs, dsts, caps, [B.ENCODE_OPTIMIZE] * n if optimize else None)
        if any(st):
            raise B.JdaError(max(st), "jda_encode_surfaces")
        return [_libjpeg_table_order(ctx.to_host(dsts[k], nbytes[k]).tobytes()) for k in range(n)]
    finally:
        ctx.free(base)


def thumbnails(ctx, files, size, quality=75, sampling="4:2:0", crops=None, prescale=None, restart_interval=0, optimize=False, resample="bilinear", progressive=False,
               pillow=False, reducing_gap=2.0):
    """files (JPEG bytes, all colour or all gray) -> list of JPEG files (bytes), each image -- or crops[k] = (x, y, w, h) of image k, in pixels
    of its visible size -- resized to size = (H, W) and encoded at `quality`; gray files take the gray sampling whatever `sampling` says.
    resample: the filter, as in decode_to_tensors (Pillow's own thumbnail() takes "bicubic").
    One Pipeline batch, one jda_resize_surfaces_ex launch and one jda_encode_surfaces call; only the files are copied back.  prescale (whole
    images only, ignored with crops): as decode_to_tensors.  optimize: every file with Huffman tables of its own (Pillow's optimize=True; a
    thumbnail loses a few hundred bytes of standard tables).  progressive: progressive files (jda_encode_surfaces_progressive: Pillow's
    progressive=True; the tables are always the file's own, so optimize changes nothing; restart_interval must be 0).  No torch in here.  A file that fails to decode raises JdaError with its status.
    prescale: None is True (what the call has always done).
    pillow=True: Pillow's own call.  size is then Pillow's (W, H) BOUND and every file gets its own final size: the returned file k is, byte
    for byte, im = Image.open(files[k]); im.thumbnail(size, F, reducing_gap); im.save(buf, "JPEG", quality=, subsampling=, optimize=,
    progressive=) -- F = resample, reducing_gap as Pillow's (None, or 0 as thumbnail_plan and decode_to_host_thumbnail take it: no draft, no reduce).  The libjpeg-exact decode at the scale draft()
    chooses, ONE jda_reduce_surfaces launch over the files that have a reduce step, ONE jda_resize_surfaces_box launch and one encode call
    with per-file sizes; a file already within size is encoded at its own size.  (A standard-table colour file's four Huffman table
    segments are put into libjpeg's order on the host: _libjpeg_table_order.)  crops and an explicit prescale=True are ValueErrors with
    it, a gray / colour mix as ever; a file the plan cannot run (jda_thumbnail_plan) raises JdaError."""
    files = list(files)
    filt = B.resize_filter(resample)
    if pillow and crops is not None:
        raise ValueError("pillow=True: Image.thumbnail takes no crop")
    if pillow and prescale:
        raise ValueError("pillow=True: the decode's scale is draft()'s, not prescale's")
    if pillow and not (reducing_gap is None or (isinstance(reducing_gap, (int, float)) and not isinstance(reducing_gap, bool) and (reducing_gap == 0 or reducing_gap >= 1.0))):
        raise ValueError("reducing_gap: None (or 0, as thumbnail_plan takes it), or a number >= 1.0 (Pillow's rule)")
    prescale = True if prescale is None else prescale
    size = tuple(int(v) for v in size)
    if len(size) != 2 or size[0] <= 0 or size[1] <= 0:
        raise ValueError("size: %s, both positive" % ("(W, H)" if pillow else "(H, W)"))
    n = len(files)
    if n == 0:
        return []
    if crops is not None:
        crops = [tuple(int(v) for v in c) for c in crops]
        if len(crops) != n or any(len(c) != 4 for c in crops):
            raise ValueError("crops: one (x, y, w, h) per file")
    infos = []
    for f in files:
        info = B.ImageInfo()
        rc = ctx.lib.jda_parse(f, len(f), C.byref(info))
        if rc != 0:
            raise B.JdaError(rc, "jda_parse")
        infos.append(info)
    gray = [i.ncomp == 1 for i in infos]
    if any(gray) != all(gray):
        raise ValueError("gray and colour files in one call: one jda_resize_surfaces launch takes one source format")
    pt = B.GRAY8 if gray[0] else B.RGB8888
    samp = B.ENCODE_GRAY if gray[0] else B.ENCODE_SAMPLINGS[sampling] if isinstance(sampling, str) else int(sampling)
    if pillow:
        return _pillow_thumbnails(ctx, files, infos, size, filt, reducing_gap, pt, samp, quality, restart_interval, optimize, progressive)
    opts = [prescale_option(i, pt, 0, size) if prescale and crops is None else 0 for i in infos]
    geos = [B.output_geometry(i, pt, o) for i, o in zip(infos, opts)]
    bpp = geos[0]["bpp"]
    pitches = [(g["canvas_w"] * bpp + 15) & ~15 for g in geos]
    offs, total = [], 0
    for g, p in zip(geos, pitches):
        offs.append(total)
        total += (p * g["canvas_h"] + 255) & ~255
    rpitch = (size[1] * bpp + 15) & ~15
    rbytes = (rpitch * size[0] + 255) & ~255
    cap = B.encode_bound_progressive(size[1], size[0], samp) if progressive else B.encode_bound(size[1], size[0], samp, restart_interval)
    base = ctx.malloc(total + rbytes * n + cap * n)
    try:
        rbase, fbase = base + total, base + total + rbytes * n
        pipe = B.Pipeline(ctx, max_images=n, depth=1)
        try:
            outs = [(base + offs[k], pitches[k], geos[k]["canvas_w"], geos[k]["canvas_h"]) for k in range(n)]
            status = pipe.wait(pipe.submit(files, outs, [pt] * n, opts))
        finally:
            pipe.close()
        for k, st in enumerate(status):
            if st != 0:
                raise B.JdaError(st, "file %d of the batch" % k)
        visible = [(base + offs[k], pitches[k], geos[k]["out_w"], geos[k]["out_h"]) for k in range(n)]
        resized = [(rbase + k * rbytes, rpitch, size[1], size[0]) for k in range(n)]
        B.resize_surfaces(ctx, visible, bpp, resized, crops, filt)
        jobs, dsts = [(0, 0, size[1], size[0], samp, quality, restart_interval)] * n, [fbase + k * cap for k in range(n)]
        if progressive:
            nbytes, st = B.encode_surfaces_progressive(ctx, resized, bpp, jobs, dsts, [cap] * n)
        else:
            nbytes, st = B.encode_surfaces(ctx, resized, bpp, jobs, dsts, [cap] * n, [B.ENCODE_OPTIMIZE] * n if optimize else None)
        if any(st):
            raise B.JdaError(max(st), "jda_encode_surfaces")
        # (the files alone come back: nbytes[k] bytes each)
        return [ctx.to_host(fbase + k * cap, nbytes[k]).tobytes() for k in range(n)]
    finally:
        ctx.free(base)
