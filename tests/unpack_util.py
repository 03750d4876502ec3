"""jda_unpack_surfaces in numpy, and the test data of tests/test_unpack_cpu.py and tests/test_gpu_unpack.py.

numpy_unpack is the twin of the kernel that knows nothing of vectors or lanes: the dense image viewed in its element type, transposed to
[h, w, C], a float element turned into a byte as np.rint(x.astype(np.float32) * s + b) in float32 (two roundings), clamped, NaN -> 0, the
channels reversed for BGR, A = 0xFF appended.  fused_unpack is the same with ONE rounding (what a fused multiply-add would give): the tests
count the elements at which the two differ, so that a kernel that contracts the product and the sum cannot pass.

grid_jobs builds the jobs of one (format, element type, parameter set): every width x height x source offset, pitches with and without 16
spare bytes, random elements with the special values of float_pool strewn over every channel."""
import functools

import numpy as np

GUARD = 0xA5
HWC, CHW, BGR = 0, 1, 2
U8, F16, F32 = 0, 1, 2
DTYPES = {U8: np.uint8, F16: np.float16, F32: np.float32}
BITS = {F16: np.uint16, F32: np.uint32}
WIDTHS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 63, 64, 65, 333)
HEIGHTS = (1, 2, 9, 217)
OFFSETS = (0, 1, 2, 3, 5, 15)                 # of the source behind a 16-byte boundary, in elements
# (destination bytes per pixel, layout flags): both layouts, BGR, the gray image under either layout word
FORMATS = ((4, HWC), (4, CHW), (4, HWC | BGR), (4, CHW | BGR), (1, HWC), (1, CHW))
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
F32_MAX = float(np.finfo(np.float32).max)


def denormalise(mean, std):
    """denormalise_params restated: [2, C] float32 = (255 * std, 255 * mean) worked out in float64"""
    return np.stack([255.0 * np.asarray(std, np.float64), 255.0 * np.asarray(mean, np.float64)]).astype(np.float32)


def param_sets(channels):
    """name -> None (the default: 255, 0) or [2, C] float32 (scale, bias)"""
    c = channels
    return {
        "default": None,
        "identity": np.array([[1.0] * c, [0.0] * c], np.float32),
        "imagenet": denormalise(IMAGENET_MEAN[:c], IMAGENET_STD[:c]),
        "negative": np.array([(-255.0, -127.5, -300.0)[:c], (255.0, 200.25, 77.5)[:c]], np.float32),
        "largest": np.array([[F32_MAX] * c, (0.0, -1e30, F32_MAX)[:c]], np.float32),
    }


def _sb(scale_bias, channels):
    if scale_bias is None:
        return np.full(channels, 255.0, np.float32), np.zeros(channels, np.float32)
    sb = np.asarray(scale_bias, np.float32).reshape(2, channels)
    return sb[0], sb[1]


def _bytes_of(t):
    """clamp(t, 0, 255) of rounded values, NaN -> 0"""
    with np.errstate(all="ignore"):
        return np.where(t >= 0, np.minimum(t, 255), 0).astype(np.uint8)


def _surface(a, bpp, flags):
    """[h, w, C] bytes in tensor channel order -> the surface's visible bytes [h, w * bpp]"""
    h, w, _ = a.shape
    if flags & BGR:
        a = a[..., ::-1]
    if bpp == 4:
        a = np.concatenate([a, np.full((h, w, 1), 255, np.uint8)], axis=2)
    return np.ascontiguousarray(a).reshape(h, w * bpp)


def _elements(src, w, h, bpp, flags, elem):
    channels = 3 if bpp == 4 else 1
    a = src.view(DTYPES[elem]).reshape((channels, h, w) if flags & CHW else (h, w, channels))
    return a.transpose(1, 2, 0) if flags & CHW else a


def numpy_unpack(src, w, h, bpp, flags, elem, scale_bias=None):
    """src: the dense image as uint8 bytes -> the visible bytes of the surface, [h, w * bpp] uint8"""
    a = _elements(src, w, h, bpp, flags, elem)
    if elem != U8:
        s, b = _sb(scale_bias, a.shape[2])
        with np.errstate(all="ignore"):
            a = _bytes_of(np.rint(a.astype(np.float32) * s + b))          # float32 * float32 + float32: two roundings
    return _surface(a, bpp, flags)


def fused_unpack(src, w, h, bpp, flags, elem, scale_bias=None):
    """numpy_unpack with the product NOT rounded: a float32 product is exact in float64, and the sum is rounded to float32 once"""
    a = _elements(src, w, h, bpp, flags, elem)
    s, b = _sb(scale_bias, a.shape[2])
    with np.errstate(all="ignore"):
        t = (a.astype(np.float64) * s.astype(np.float64) + b.astype(np.float64)).astype(np.float32)
        return _surface(_bytes_of(np.rint(t)), bpp, flags)


def _f32_bits(values):
    return np.asarray(values, np.float32).view(np.uint32)


def contraction_values(s, b, elem=F32):
    """the x at which rint(x * s + b) differs between two roundings and one, as bit patterns: of the float32 values near every tie
    (k + 0.5 - b) / s, or of ALL float16 values"""
    if not np.isfinite(s) or s == 0 or b == 0:
        return np.zeros(0, BITS[elem])
    with np.errstate(all="ignore"):
        if elem == F16:
            x = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
        else:
            x0 = ((np.arange(-1, 256, dtype=np.float64) + 0.5 - float(b)) / float(s)).astype(np.float32)
            x = (x0.view(np.int32)[:, None] + np.arange(-48, 49, dtype=np.int32)[None, :]).reshape(-1).view(np.float32)
        bits = x.view(BITS[elem])
        keep = np.isfinite(x)
        x, bits = x[keep].astype(np.float32), bits[keep]
        two = _bytes_of(np.rint(x * np.float32(s) + np.float32(b)))
        one = _bytes_of(np.rint((x.astype(np.float64) * float(s) + float(b)).astype(np.float32)))
    return bits[two != one]


@functools.lru_cache(maxsize=None)
def _float_pool(elem, s, b):
    return float_pool(elem, np.float32(s), np.float32(b))


def float_pool(elem, s, b):
    """bit patterns every float test image holds in the channel with scale s and bias b: quiet and signalling NaNs, +-inf, +-0, subnormals of
    both types, every k + 0.5 for k = -1 .. 255 and what gives it under (s, b), values above 3e38, and the contraction set"""
    halves = np.arange(-1, 256, dtype=np.float64) + 0.5
    with np.errstate(all="ignore"):
        pre = (halves - float(b)) / float(s) if s != 0 else halves
    if elem == F16:
        fixed = np.array([0x7e00, 0xfe00, 0x7c01, 0xfd55, 0x7fff, 0x7c00, 0xfc00, 0x0000, 0x8000, 0x0001, 0x8001, 0x03ff, 0x83ff, 0x0200, 0x7bff, 0xfbff, 0x3c00], np.uint16)
        with np.errstate(all="ignore"):
            return np.concatenate([fixed, halves.astype(np.float16).view(np.uint16), pre.astype(np.float16).view(np.uint16), contraction_values(s, b, F16)])
    fixed = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffa00000, 0x7fffffff, 0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
                      0x007fffff, 0x807fffff, 0x00400000], np.uint32)
    with np.errstate(all="ignore"):
        more = np.concatenate([_f32_bits([3.1e38, -3.1e38, F32_MAX, -F32_MAX, 2.0 ** -24, 2.0 ** -15 * 1.5, -(2.0 ** -24)]), _f32_bits(halves), _f32_bits(pre)])
    return np.concatenate([fixed, more, contraction_values(s, b)])


def random_image(rng, w, h, channels, elem, scale_bias, turn=0):
    """[h, w, C] random elements (float: random bit patterns, mostly values that land in and around 0 .. 255, and the pool of every
    channel strewn over it, beginning at pool entry `turn` so that small images get through the pool between them)"""
    if elem == U8:
        return rng.randint(0, 256, (h, w, channels)).astype(np.uint8)
    s, b = _sb(scale_bias, channels)
    img = np.empty((h, w, channels), BITS[elem])
    for c in range(channels):
        with np.errstate(all="ignore"):
            near = ((rng.uniform(-40.0, 300.0, h * w) - float(b[c])) / (float(s[c]) if s[c] != 0 else 1.0)).astype(DTYPES[elem]).view(BITS[elem])
        wild = rng.randint(0, 1 << 16, h * w).astype(BITS[elem]) if elem == F16 else (rng.randint(0, 1 << 16, h * w).astype(np.uint32) << 16) | rng.randint(0, 1 << 16, h * w).astype(np.uint32)
        plane = np.where(rng.randint(0, 4, h * w) == 0, wild, near)
        pool = _float_pool(elem, float(s[c]), float(b[c]))
        k = min(h * w, len(pool))
        plane[rng.permutation(h * w)[:k]] = np.roll(pool, -(turn * 7) % len(pool))[:k]
        img[:, :, c] = plane.reshape(h, w)
    return img.view(DTYPES[elem])


def dense_bytes(img, flags):
    """[h, w, C] elements -> the dense image in its layout, as bytes"""
    a = img.transpose(2, 0, 1) if flags & CHW else img
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def grid_jobs(rng, bpp, flags, elem, scale_bias):
    """every width x height x source offset of the grid: dicts with w, h, offset (bytes behind a 16-byte boundary: the element multiples of OFFSETS), pitch, src (bytes),
    want (the twin's visible bytes, [h, w * bpp]), fused_differs (elements at which a fused multiply-add gives another byte)"""
    channels, es = (3 if bpp == 4 else 1), np.dtype(DTYPES[elem]).itemsize
    jobs = []
    for w in WIDTHS:
        for h in HEIGHTS:
            for off in OFFSETS:
                k = len(jobs)
                img = random_image(rng, w, h, channels, elem, scale_bias, k)
                src = dense_bytes(img, flags)
                want = numpy_unpack(src, w, h, bpp, flags, elem, scale_bias)
                differs = 0 if elem == U8 else int(np.count_nonzero(want != fused_unpack(src, w, h, bpp, flags, elem, scale_bias)))
                jobs.append({"w": w, "h": h, "offset": off * es, "pitch": ((w * bpp + 15) & ~15) + 16 * (k & 1), "src": src, "want": want, "fused_differs": differs})
    return jobs
