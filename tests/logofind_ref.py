"""numpy statement of the automatic logo finder's sums and of its rectangle rule, for the tests."""
import numpy as np


def sums(Y, W, H):
    """Y: (N, H, >= W) samples -> 2*W*H int64: S1 = sum Y, then SM = sum |Y[x+1] - Y[x-1]| + |Y[y+1] - Y[y-1]| (0 on the outer ring)"""
    Y = np.asarray(Y)[:, :H, :W].astype(np.int64)
    S1 = Y.sum(0)
    SM = np.zeros_like(S1)
    if Y.shape[0]:
        SM[1:-1, 1:-1] = (np.abs(Y[:, 1:-1, 2:] - Y[:, 1:-1, :-2]) + np.abs(Y[:, 2:, 1:-1] - Y[:, :-2, 1:-1])).sum(0)
    return np.concatenate([S1.ravel(), SM.ravel()])


def rect_of_box(bx0, by0, bx1, by1, W, H, margin=4):
    """the rectangle of an edge-pixel bounding box (inclusive corners): grown by `margin`, corner rounded down to even, size up to even,
    clipped to the frame"""
    x0, y0 = max(0, bx0 - margin) & ~1, max(0, by0 - margin) & ~1
    x1, y1 = min(W, bx1 + 1 + margin), min(H, by1 + 1 + margin)
    w, h = (x1 - x0 + 1) & ~1, (y1 - y0 + 1) & ~1
    if x0 + w > W:
        w -= 2
    if y0 + h > H:
        h -= 2
    return x0, y0, w, h
