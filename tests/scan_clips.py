"""Clips for the LogoScan tests: random noise everywhere, and around the scan rectangle of every plane a border ring whose spread
(max - min) is chosen per frame and per plane, so that a test can sit exactly on the `abs(min - max) <= thy` edge."""
import numpy as np


def _ring_index(w, h):
    m = np.zeros((h, w), bool)
    m[0] = m[-1] = True
    m[:, 0] = m[:, -1] = True
    return np.flatnonzero(m.ravel())


def make_scan_clip(rng, W, H, pad, bits, rect, plan, container_max=None):
    """rect = (x, y, w, h) in luma samples.  plan: one entry per frame, {"spread": (sY, sU, sV), "base": (bY, bU, bV) or absent}.
    The ring of plane k holds base + randint(0 .. spread) with both ends present (a one-sample ring can only have spread 0); a missing
    base is drawn so that the ring stays inside the declared depth.  Returns (clip, info): clip = {"Y", "U", "V"} arrays of shape
    (n, rows, pitch), uint8 or uint16; info[i] = ((base, realised spread) for Y, U, V)."""
    x0, y0, w, h = rect
    maxv = (1 << bits) - 1
    hi = maxv if container_max is None else container_max
    dt = np.uint8 if bits <= 8 else np.uint16
    n = len(plan)
    pY, pUV = W + pad, W // 2 + pad // 2
    clip = {"Y": rng.randint(0, maxv + 1, (n, H, pY)).astype(dt),
            "U": rng.randint(0, maxv + 1, (n, H // 2, pUV)).astype(dt),
            "V": rng.randint(0, maxv + 1, (n, H // 2, pUV)).astype(dt)}
    geo = {"Y": (x0, y0, w, h), "U": (x0 // 2, y0 // 2, w // 2, h // 2), "V": (x0 // 2, y0 // 2, w // 2, h // 2)}
    rings = {k: _ring_index(g[2], g[3]) for k, g in geo.items()}
    info = []
    for i, fr in enumerate(plan):
        rec = []
        for k, name in enumerate("YUV"):
            px, py, pw, ph = geo[name]
            idx = rings[name]
            spread = int(fr["spread"][k]) if idx.size > 1 else 0
            base = fr["base"][k] if fr.get("base") is not None else int(rng.randint(0, hi - spread + 1))
            assert 0 <= base and base + spread <= hi
            block = clip[name][i, py:py + ph, px:px + pw].copy().ravel()
            vals = base + rng.randint(0, spread + 1, idx.size)
            if idx.size > 1:
                a, b = rng.choice(idx.size, 2, replace=False)
                vals[a], vals[b] = base, base + spread
            block[idx] = vals
            clip[name][i, py:py + ph, px:px + pw] = block.reshape(ph, pw)
            rec.append((base, spread))
        info.append(tuple(rec))
    return clip, info
