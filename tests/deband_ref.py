"""numpy restatement of the deband rule (include/amt_gpu.h, amtgpu_deband_*), written from the rule's text: the
offset table of a plane and the filter of a plane and of a clip.  Integer throughout; nothing here knows how the kernel works."""
import numpy as np

M32 = 0xFFFFFFFF


def mix(v):
    """the 32-bit finaliser on uint64 arrays holding uint32 values"""
    v = np.asarray(v, np.uint64) & M32
    v ^= v >> 16
    v = (v * 0x7FEB352D) & M32
    v ^= v >> 15
    v = (v * 0x846CA68B) & M32
    v ^= v >> 16
    return v


def plane_radius(plane, radius):
    return radius >> 1 if plane else radius


def plane_size(plane, w, h):
    return (w >> 1, h >> 1) if plane else (w, h)


def lim_map(W, H, R):
    x, y = np.arange(W)[None, :], np.arange(H)[:, None]
    return np.minimum(np.minimum(np.minimum(x, W - 1 - x), np.minimum(y, H - 1 - y)), R).astype(np.int64)


def table(plane, W, H, R, seed=0):
    """(dx, dy) of plane `plane` of W x H containers with the PLANE's radius R, int8 (H, W)"""
    lim = lim_map(W, H, R)
    key = mix(np.uint64((seed + 0x9E3779B9 * (plane + 1)) & M32))
    x, y = np.arange(W, dtype=np.uint64)[None, :], np.arange(H, dtype=np.uint64)[:, None]
    h = mix(key ^ ((y << 16) | x))
    a, b = (h & 255).astype(np.int64), ((h >> 8) & 255).astype(np.int64)
    dx = ((a * (2 * lim + 1)) >> 8) - lim
    dy = ((b * (2 * lim + 1)) >> 8) - lim
    return dx.astype(np.int8), dy.astype(np.int8)


def references(s, dx, dy):
    """(c, [p0, p1, p2, p3]) as int64 arrays shaped like s: (H, W) or (N, H, W)"""
    H, W = s.shape[-2:]
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    dx, dy = dx.astype(np.int64), dy.astype(np.int64)
    S = s.astype(np.int64)
    return S, [S[..., y + dy, x + dx], S[..., y - dy, x - dx], S[..., y + dx, x - dy], S[..., y - dx, x + dy]]


def filter_plane(s, dx, dy, thresh, sample=2, blur_first=True):
    """thresh: threshold << (bits - 8).  Containers as stored"""
    c, p = references(s, dx, dy)
    if sample == 0:
        avg, p = p[0], p[:1]
    elif sample == 1:
        avg, p = (p[0] + p[1] + 1) >> 1, p[:2]
    else:
        avg = (p[0] + p[1] + p[2] + p[3] + 2) >> 2
    if blur_first or sample == 0:
        take = np.abs(avg - c) <= thresh
    else:
        take = np.all([np.abs(q - c) <= thresh for q in p], axis=0)
    return np.where(take, avg, c).astype(s.dtype)


def tables(w, h, radius, seed=0):
    """the three planes' (dx, dy) of a w x h clip"""
    return [table(p, *plane_size(p, w, h), plane_radius(p, radius), seed) for p in range(3)]


def filter_clip(planes, bits, radius=25, threshold=1, sample=2, blur_first=True, seed=0, offsets=None):
    """planes: (Y, U, V), each (N, Hp, Wp); offsets: the three planes' (dx, dy) where they are not the rule's"""
    h, w = planes[0].shape[-2:]
    if offsets is None:
        offsets = tables(w, h, radius, seed)
    return tuple(filter_plane(s, dx, dy, threshold << (bits - 8), sample, blur_first) for s, (dx, dy) in zip(planes, offsets))
