"""numpy restatement of the edge level's rule (include/amt_gpu.h, "edge level"), written from the rule's text and
not from the kernel: whole planes at a time, every step of the text one line below, the nine samples of the repair sorted with np.sort.
Also the clips the CPU and GPU tests share."""
import functools

import numpy as np

DEFAULTS = (16, 10, 2)                                                  # the server's KEdgeLevel(16, 10, 2)
FLAT, SHARP, BLURRED, LEVELLED = "flat", "sharp", "blurred", "levelled"


def classify(s, bits, threshold):
    """the interior of one luma plane s (H, W), H, W >= 5, as int64 arrays over (H - 4, W - 4): dict of c, vertical (bool), mx, mn, rng, step
    and the four classes (bool each, exactly one true per pixel)"""
    s = np.asarray(s).astype(np.int64)
    H, W = s.shape
    T = int(threshold) << (bits - 8)
    H5 = np.stack([s[2:H - 2, 2 + j:W - 2 + j] for j in range(-2, 3)])           # s[y][x-2 .. x+2]
    V5 = np.stack([s[2 + j:H - 2 + j, 2:W - 2] for j in range(-2, 3)])           # s[y-2 .. y+2][x]
    rh, rv = H5.max(0) - H5.min(0), V5.max(0) - V5.min(0)
    vertical = rh < rv                                                  # a tie takes the horizontal line
    L = np.where(vertical[None], V5, H5)
    mx, mn = L.max(0), L.min(0)
    rng = mx - mn
    step = np.abs(np.diff(L, axis=0)).max(0)
    flat = rng <= T
    sharp = ~flat & (4 * step >= 3 * rng)
    blurred = ~flat & ~sharp & (8 * step <= 3 * rng)
    return dict(c=L[2], vertical=vertical, mx=mx, mn=mn, rng=rng, step=step, flat=flat, sharp=sharp, blurred=blurred, levelled=~flat & ~sharp & ~blurred)


def filter_plane(s, bits, strength=16, threshold=10, repair=2):
    """one luma plane (H, W) -> the filtered plane, same dtype"""
    s = np.asarray(s)
    H, W = s.shape
    out = s.copy()
    if H < 5 or W < 5:
        return out                                                      # all border
    k = classify(s, bits, threshold)
    c, mx, mn = k["c"], k["mx"], k["mn"]
    avg = (mx + mn) >> 1
    e = c + (((c - avg) * int(strength)) >> 4)                          # numpy's >> on int64 is arithmetic: floor
    e = np.clip(e, mn, mx)
    if repair > 0:
        q = s.astype(np.int64)
        nine = np.sort(np.stack([q[1 + dy:H - 3 + dy, 1 + dx:W - 3 + dx] for dy in range(3) for dx in range(3)]), axis=0)    # s[y-1..y+1][x-1..x+1]
        e = np.minimum(np.maximum(e, nine[repair - 1]), nine[9 - repair])
    out[2:H - 2, 2:W - 2] = np.where(k["levelled"], e, c).astype(s.dtype)
    return out


def filter_clip(planes, bits, strength=16, threshold=10, repair=2):
    """(Y, U, V), each (n, h, w) -> the same: luma filtered frame by frame, chroma as stored"""
    Y, U, V = planes
    return np.stack([filter_plane(f, bits, strength, threshold, repair) for f in Y]), U.copy(), V.copy()


def shares(s, bits, threshold=10, strength=16):
    """shares of the interior: the four classes, the vertical line, and the pixels repair 2 moves against repair 0"""
    k = classify(s, bits, threshold)
    H, W = np.asarray(s).shape
    r0, r2 = filter_plane(s, bits, strength, threshold, 0), filter_plane(s, bits, strength, threshold, 2)
    out = {name: float(k[name].mean()) for name in (FLAT, SHARP, BLURRED, LEVELLED)}
    out["vertical"] = float(k["vertical"].mean())
    out["repaired"] = float((r0 != r2)[2:H - 2, 2:W - 2].mean())
    return out


def blur121(p, axis):
    """[1 2 1] / 4 with rounding along one axis, edges replicated"""
    p = np.moveaxis(p, axis, -1)
    q = np.concatenate([p[..., :1], p, p[..., -1:]], axis=-1)
    return np.moveaxis((q[..., :-2] + 2 * q[..., 1:-1] + q[..., 2:] + 2) >> 2, -1, axis)


def soft_plane(rng, n, ph, pw, content):
    """blocks of 6 x 6 of 16..235 (in 8-bit units), two passes of the blur along each axis, noise of 0..2 units on top"""
    u = 1 << (content - 8)
    by, bx = (ph + 5) // 6, (pw + 5) // 6
    p = np.repeat(np.repeat(rng.integers(16, 236, (n, by, bx)), 6, axis=1), 6, axis=2)[:, :ph, :pw].astype(np.int64) * u
    for _ in range(2):
        p = blur121(blur121(p, 2), 1)
    return p + rng.integers(0, 2 * u + 1, (n, ph, pw))


@functools.lru_cache(maxsize=None)
def clip(w, h, depth, kind, n=2):
    """depth: (bits, bits of the content).  random: every container uniform over the content's range.  soft: soft_plane.  Chroma planes
    are uniform random either way (they are copied).  The arrays are read-only and shared"""
    bits, content = depth
    dt = np.uint8 if bits <= 8 else np.uint16
    rng = np.random.default_rng(w * 977 + h * 31 + content)
    planes = []
    for k, (pw, ph) in enumerate(((w, h), (w // 2, h // 2), (w // 2, h // 2))):
        p = soft_plane(rng, n, ph, pw, content) if kind == "soft" and k == 0 else rng.integers(0, 1 << content, (n, ph, pw))
        p = p.astype(dt)
        p.setflags(write=False)
        planes.append(p)
    return tuple(planes)


# ---- planted pixels: a 9 x 9 plane whose pixel (4, 4) sits on a boundary of the rule, or one beyond ----
def planted_line(line, vertical=False, base=None, dt=np.uint8, size=9):
    """a plane of `base` (default: line[2]) whose row (column, if vertical) through the centre holds `line` in its middle five"""
    s = np.full((size, size), line[2] if base is None else base, dt)
    m = size // 2
    if vertical:
        s[m - 2:m + 3, m] = line
    else:
        s[m, m - 2:m + 3] = line
    return s


def boundary_lines(bits, threshold=10):
    """{name: (line of five, does the centre pixel change under strength 16, repair 0)}: each boundary of the rule and one beyond it"""
    u = 1 << (bits - 8)
    T = threshold << (bits - 8)
    b = 50 * u
    out = {
        # rng == T (flat) and T + 1 (levelled: step T / 2 + 1 .. of rng T + 1 lies between 3/8 and 3/4 of it)
        "rng == T": ([b, b, b + T // 2 - u, b + T, b + T], False),
        "rng == T + 1": ([b, b, b + T // 2 - u, b + T + 1, b + T + 1], True),
        # 4 step == 3 rng: rng 40 u, step 30 u (sharp); one less: step 30 u - 1
        "4 step == 3 rng": ([b, b, b + 10 * u, b + 40 * u, b + 40 * u], False),
        "4 step == 3 rng - 1": ([b, b, b + 10 * u + 1, b + 40 * u, b + 40 * u], True),
        # 8 step == 3 rng: rng 64 u, step 24 u (too blurred); one more: step 24 u + 1
        "8 step == 3 rng": ([b, b + 8 * u, b + 24 * u, b + 48 * u, b + 64 * u], False),
        "8 step == 3 rng + 1": ([b, b + 8 * u, b + 24 * u - 1, b + 48 * u, b + 64 * u], True),
    }
    return out
