"""AMTGPU_ANALYZE_LINEAR_MONITORED: the guarded linear mode with K exact sentinel frames per batch, compared with their linear scores on
the device; a failed comparison re-evaluates the batch exactly and keeps the analyzer exact until it is re-armed.

Every expectation is computed here from the other modes on the same data: the exact mode's records, mode 1's ("linear") and the
linear kernel's own values ("linear_unguarded", which is what the monitor compares before the guard touches anything)."""
import threading

import numpy as np
import pytest

import amt_synth as S
from test_gpu_parity import SMALL, gpu, make_case  # noqa: F401  (fixture + helpers)

pytestmark = pytest.mark.gpu


def sentinels(n, k=16):
    k = min(k, n)
    return [0] if k == 1 else [j * (n - 1) // (k - 1) for j in range(k)]


def run_modes(gpu, logo, dclip, maskratio=0.35):
    """records of the exact mode, of mode 1, of the unguarded linear kernel, mode 1's last_refined and its error bounds"""
    from amatsukaze_amd import AMTAnalyzeLogo
    ctx = gpu["ctx"]
    exact = AMTAnalyzeLogo(ctx, logo, maskratio).analyze(dclip)
    lin = AMTAnalyzeLogo(ctx, logo, maskratio, mode="linear")
    m1 = lin.analyze(dclip)
    raw = AMTAnalyzeLogo(ctx, logo, maskratio, mode="linear_unguarded").analyze(dclip)
    bounds = [lin.error_bound(k, dclip.bits) for k in range(3)]
    return dict(exact=exact, m1=m1, raw=raw, m1_refined=lin.last_refined(), bounds=bounds)


def guard_listed(raw, bounds):
    """the frames analysis_mark_kernel lists from the linear records: NaN in a group, or best / second best not 2x the bound apart"""
    amb = np.zeros(raw.shape[0], bool)
    for k in range(3):
        g = raw[:, 11 * k:11 * k + 11]
        srt = np.sort(g, axis=1)
        eps = np.float32(2.0) * np.float32(bounds[k])
        amb |= np.isnan(g).any(axis=1) | ~((srt[:, 1] - srt[:, 0]) > eps)
    return amb


def sentinel_max(raw, exact, rows):
    return float(np.abs(raw[rows] - exact[rows]).max()) if len(rows) else 0.0


def adversarial_case(gpu, n, seed=0x5EED0031):
    """the strong logo of test_linear_mode_under_adversarial_coefficients (alpha up to 0.9)"""
    from amatsukaze_amd import DeviceClip, Logo
    torch = gpu["torch"]
    W, H, LW, LH, X, Y0 = 352, 240, 96, 48, 224, 18
    data, alpha, alphaUV = S.make_logo(LW, LH, strength=1.5)
    clip = S.make_clip_np(n, W, H, seed, alpha, alphaUV, X, Y0, bits=8, period=5, fade=3, flat_every=4)
    dclip = DeviceClip(*(torch.from_numpy(clip[k]).to(gpu["dev"]) for k in "YUV"), width=W, height=H, bits=8)
    return Logo.from_planes(gpu["ctx"], data, LW, LH, W, H, X, Y0), dclip


def tripping_case(gpu, n=200):
    """a clip whose sentinels show a nonzero linear error (the plain case, or the adversarial logo when the plain one is exact there)"""
    cs = make_case(gpu, dict(SMALL, N=n), bits=8, pitch_pad=32)
    logo, dclip = cs["logo"], cs["dclip"]
    r = run_modes(gpu, logo, dclip)
    if sentinel_max(r["raw"], r["exact"], sentinels(n)) == 0.0:
        logo, dclip = adversarial_case(gpu, n)
        r = run_modes(gpu, logo, dclip)
    smax = sentinel_max(r["raw"], r["exact"], sentinels(n))
    assert smax > 0.0
    return logo, dclip, r, smax


@pytest.mark.parametrize("bits", [8, 10])
def test_passing_batch(gpu, bits):
    """default tolerance and sentinels on a plain clip: no downgrade, 16 frames compared, the max is the sentinels' own |linear - exact|,
    sentinel rows carry the exact bytes and every other row mode 1's"""
    from amatsukaze_amd import AMTAnalyzeLogo
    n = 200
    cs = make_case(gpu, dict(SMALL, N=n), bits=bits, pitch_pad=32)
    r = run_modes(gpu, cs["logo"], cs["dclip"])
    mon = AMTAnalyzeLogo(gpu["ctx"], cs["logo"], 0.35, mode="monitored")
    got = mon.analyze(cs["dclip"])
    st = mon.monitor_stats()
    sent = sentinels(n)
    assert not st["downgraded"] and st["frames_checked"] == 16, st
    want_max = sentinel_max(r["raw"], r["exact"], sent)
    assert st["max_abs"] <= 1e-4 and st["max_abs"] == np.float32(want_max), (st, want_max)
    other = np.setdiff1d(np.arange(n), sent)
    assert got[sent].tobytes() == r["exact"][sent].tobytes()
    assert got[other].tobytes() == r["m1"][other].tobytes()
    listed = guard_listed(r["raw"], r["bounds"])
    assert r["m1_refined"] == int(listed.sum())
    listed[sent] = True
    assert mon.last_refined() == int(listed.sum())
    assert mon.error_bound(0, bits) == AMTAnalyzeLogo(gpu["ctx"], cs["logo"], 0.35, mode="linear").error_bound(0, bits) > 0


def test_tripping_downgrades_and_rearms(gpu):
    from amatsukaze_amd import AMTAnalyzeLogo, AMTEraseLogo
    ctx = gpu["ctx"]
    n = 200
    logo, dclip, r, smax = tripping_case(gpu, n)
    er = AMTEraseLogo(ctx, logo, "", 0, 16)
    mon = AMTAnalyzeLogo(ctx, logo, 0.35, mode="monitored", tolerance=smax / 2)
    got = mon.analyze(dclip)
    assert got.tobytes() == r["exact"].tobytes()
    st = mon.monitor_stats()
    assert st["downgraded"] and st["frames_checked"] == 16 and st["max_abs"] == np.float32(smax), st
    assert mon.last_refined() == n
    assert mon.error_bound(0, 8) == 0.0
    assert er.calc_fades(got, n).tobytes() == er.calc_fades(r["exact"], n).tobytes()
    # a later batch, another clip and size (several frames per workgroup in the exact pass): exact, all of it
    n2 = 1400
    cs2 = make_case(gpu, dict(SMALL, N=n2), bits=8, seed=0x5EED0077)
    exact2 = AMTAnalyzeLogo(ctx, logo, 0.35).analyze(cs2["dclip"])
    got2 = mon.analyze(cs2["dclip"])
    assert got2.tobytes() == exact2.tobytes()
    assert mon.last_refined() == n2
    assert mon.monitor_stats()["downgraded"]
    # re-arming clears the downgrade and the statistics; the next batch is linear again
    mon.set_monitor(1.0, 16)
    mon.set_mode("monitored")
    assert mon.monitor_stats() == {"max_abs": 0.0, "frames_checked": 0, "downgraded": False}
    got3 = mon.analyze(dclip)
    sent = sentinels(n)
    other = np.setdiff1d(np.arange(n), sent)
    assert got3[other].tobytes() == r["m1"][other].tobytes()
    assert got3[sent].tobytes() == r["exact"][sent].tobytes()
    assert mon.last_refined() < n
    st = mon.monitor_stats()
    assert not st["downgraded"] and st["frames_checked"] == 16
    assert er.calc_fades(got3, n).tobytes() == er.calc_fades(r["exact"], n).tobytes()
    # any other mode turns the monitor off
    mon.set_mode("linear")
    assert mon.analyze(dclip).tobytes() == r["m1"].tobytes()


def test_device_state_is_the_source_of_truth(gpu):
    """batches enqueued back to back without any host wait: the one that trips and every one after it are exact, whenever the host
    notices"""
    from amatsukaze_amd import AMTAnalyzeLogo
    torch = gpu["torch"]
    n = 200
    logo, dclip, r, smax = tripping_case(gpu, n)
    mon = AMTAnalyzeLogo(gpu["ctx"], logo, 0.35, mode="monitored", tolerance=smax / 2)
    outs = [torch.empty((n, 33), dtype=torch.float32, device=gpu["dev"]) for _ in range(3)]
    for o in outs:
        mon.analyze_device(dclip.Y, 8, o)
    gpu["ctx"].synchronize()
    for o in outs:
        assert o.cpu().numpy().tobytes() == r["exact"].tobytes()
    assert mon.monitor_stats()["downgraded"]


def test_generous_tolerance_accumulates(gpu):
    """tolerance twice the largest error over ALL frames: never trips; statistics accumulate over batches"""
    from amatsukaze_amd import AMTAnalyzeLogo
    n = 200
    cases = [make_case(gpu, dict(SMALL, N=n), bits=8, seed=s) for s in (0x5EED0001, 0x5EED0002, 0x5EED0003)]
    runs = [run_modes(gpu, c["logo"], c["dclip"]) for c in cases]
    worst = max(float(np.abs(x["raw"] - x["exact"]).max()) for x in runs)
    mon = AMTAnalyzeLogo(gpu["ctx"], cases[0]["logo"], 0.35, mode="monitored", tolerance=2 * worst)
    sent = sentinels(n)
    for c, x in zip(cases, runs):
        got = mon.analyze(c["dclip"])
        other = np.setdiff1d(np.arange(n), sent)
        assert got[other].tobytes() == x["m1"][other].tobytes()
    st = mon.monitor_stats()
    assert not st["downgraded"] and st["frames_checked"] == 16 * len(cases)
    assert st["max_abs"] == np.float32(max(sentinel_max(x["raw"], x["exact"], sent) for x in runs)), st


@pytest.mark.parametrize("n,k", [(40, 1), (40, 40), (40, 64), (1, 16), (17, 16)])
def test_sentinel_edges(gpu, n, k):
    from amatsukaze_amd import AMTAnalyzeLogo
    cs = make_case(gpu, dict(SMALL, N=n), bits=8)
    r = run_modes(gpu, cs["logo"], cs["dclip"])
    mon = AMTAnalyzeLogo(gpu["ctx"], cs["logo"], 0.35, mode="monitored", sentinels=k)
    got = mon.analyze(cs["dclip"])
    sent = sentinels(n, k)
    assert len(set(sent)) == min(n, k) and sent[0] == 0 and sent[-1] == (n - 1 if min(n, k) > 1 else 0)
    st = mon.monitor_stats()
    assert not st["downgraded"] and st["frames_checked"] == len(sent), st
    assert st["max_abs"] == np.float32(sentinel_max(r["raw"], r["exact"], sent))
    other = np.setdiff1d(np.arange(n), sent)
    assert got[sent].tobytes() == r["exact"][sent].tobytes()
    assert got[other].tobytes() == r["m1"][other].tobytes()
    if k >= n:
        assert got.tobytes() == r["exact"].tobytes() and mon.last_refined() == n


def test_out_of_range_sentinels_are_not_compared(gpu):
    """10-bit samples above maxv on sentinel frames (the set-up of test_linear_mode_hands_out_of_range_samples_to_the_exact_kernel): the
    frames are exact anyway, they neither trip the monitor nor count as compared"""
    from amatsukaze_amd import AMTAnalyzeLogo, DeviceClip
    cfg = dict(W=352, H=240, LW=96, LH=48, IMGX=224, IMGY=18, N=24, period=6, fade=3, flat=3)
    cs = make_case(gpu, cfg, bits=10, pitch_pad=32)
    dc = cs["dclip"]
    Y = dc.Y.clone()
    sent = sentinels(cfg["N"])
    dirty = [sent[0], sent[5], sent[-1]]
    for n in dirty:
        Y[n, cfg["IMGY"] + 5 + n % 7, cfg["IMGX"] + 9 + 2 * n] = 3000 + n
    clip = DeviceClip(Y, dc.U, dc.V, dc.width, dc.height, 10)
    exact = AMTAnalyzeLogo(gpu["ctx"], cs["logo"], 0.35).analyze(clip)
    mon = AMTAnalyzeLogo(gpu["ctx"], cs["logo"], 0.35, mode="monitored")
    got = mon.analyze(clip)
    st = mon.monitor_stats()
    assert not st["downgraded"] and st["frames_checked"] == len(sent) - len(dirty), st
    assert st["max_abs"] <= 1e-4
    for n in dirty:
        assert got[n].tobytes() == exact[n].tobytes(), n
    assert got[sent].tobytes() == exact[sent].tobytes()


@pytest.mark.parametrize("trip", [False, True])
def test_device_output_path(gpu, trip):
    """analyze_device -> calc_fades_device in the monitored mode, no host round trip: fades identical to the exact mode's"""
    from amatsukaze_amd import AMTAnalyzeLogo, AMTEraseLogo
    torch = gpu["torch"]
    n = 200
    logo, dclip, r, smax = tripping_case(gpu, n)
    er = AMTEraseLogo(gpu["ctx"], logo, "", 0, 16)
    mon = AMTAnalyzeLogo(gpu["ctx"], logo, 0.35, mode="monitored", tolerance=smax / 2 if trip else 1e-4)
    d_rec = torch.empty((n, 33), dtype=torch.float32, device=gpu["dev"])
    mon.analyze_device(dclip.Y, 8, d_rec)
    d_f = er.calc_fades_device(d_rec, n)
    gpu["ctx"].synchronize()
    assert d_f.cpu().numpy().tobytes() == er.calc_fades(r["exact"], n).tobytes()
    assert mon.monitor_stats()["downgraded"] == trip
    if trip:
        assert d_rec.cpu().numpy().tobytes() == r["exact"].tobytes()


def test_argument_errors(gpu):
    from amatsukaze_amd import AMTAnalyzeLogo, AmtError
    cs = make_case(gpu, dict(SMALL, N=40), bits=8)
    ctx = gpu["ctx"]
    mon = AMTAnalyzeLogo(ctx, cs["logo"], 0.35, mode="monitored")
    for tol, k in [(-1e-4, 16), (float("nan"), 16), (float("inf"), 16), (1e-4, 0), (1e-4, -3)]:
        assert ctx.lib.amtgpu_analyze_set_monitor(mon.h, tol, k) == 0
        assert ctx.lib.amtgpu_last_error(ctx.h).decode().startswith("monitor:")
        with pytest.raises(AmtError):
            mon.set_monitor(tol, k)
    with pytest.raises(AmtError):
        AMTAnalyzeLogo(ctx, cs["logo"], 0.35, mode="monitored", sentinels=0)
    assert ctx.lib.amtgpu_analyze_set_monitor(mon.h, 0.0, 1) == 1          # 0: any difference trips
    assert ctx.lib.amtgpu_analyze_set_monitor(mon.h, 1e-4, 16) == 1
    exact = AMTAnalyzeLogo(ctx, cs["logo"], 0.35).analyze(cs["dclip"])
    got = mon.analyze(cs["dclip"])
    st = mon.monitor_stats()
    assert st["frames_checked"] == 16 and not st["downgraded"]
    assert np.abs(got - exact).max() <= 1e-4
    assert ctx.lib.amtgpu_analyze_monitor_stats(mon.h, None, None, None) == 1


def test_two_threads_one_monitored_analyzer(gpu):
    """two host threads drive one monitored analyzer through one context; one of them trips it.  Every batch is the exact mode's
    records, or a passing batch's (sentinels exact, the rest mode 1's); the statistics are whole batches"""
    from amatsukaze_amd import AMTAnalyzeLogo
    n = 200
    logo, dclip, r, smax = tripping_case(gpu, n)
    mon = AMTAnalyzeLogo(gpu["ctx"], logo, 0.35, mode="monitored", tolerance=1.0)
    sent = sentinels(n)
    other = np.setdiff1d(np.arange(n), sent)
    results, errors = [], []
    lock = threading.Lock()

    def worker(k):
        try:
            for it in range(6):
                if k == 1 and it == 2:
                    mon.set_monitor(smax / 2, 16)
                got = mon.analyze(dclip)
                with lock:
                    results.append(got)
        except Exception as e:           # pragma: no cover - reported below
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert len(results) == 12
    for got in results:
        passing = got[sent].tobytes() == r["exact"][sent].tobytes() and got[other].tobytes() == r["m1"][other].tobytes()
        assert got.tobytes() == r["exact"].tobytes() or passing
    st = mon.monitor_stats()
    assert st["downgraded"]
    assert st["frames_checked"] % 16 == 0 and 16 <= st["frames_checked"] <= 16 * 12, st
    assert st["max_abs"] == np.float32(smax)
    assert results[-1].tobytes() == r["exact"].tobytes()
