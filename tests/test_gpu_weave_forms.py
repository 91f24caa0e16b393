"""weave_fields_kernel (amtgpu_weave_fields_batch, amtgpu_weave_fields_batch_msb) on every form the host selects -- 16-byte vectors
with and without a partial vector at the end of a row, single elements because of a pitch, a base or a frame stride, the NV12 split,
both kernels at two bytes per sample -- against the definition in numpy (tests/copy_cases.py, judged by
tests/test_copy_cases_host.py).  The planes are flat buffers with guards, padding and frame gaps at a sentinel; every byte of the
destination is compared, and the sources with what was uploaded."""
import ctypes as C

import pytest

import copy_cases as K

pytestmark = pytest.mark.gpu

BY_NAME = {c.name: c for c in K.WEAVE_CASES}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from amatsukaze_amd import Context
    return dict(torch=torch, ctx=Context(0), dev=torch.device("cuda:0"))


def upload(gpu, bufs):
    out = {w: gpu["torch"].from_numpy(b).to(gpu["dev"]) for w, b in bufs.items()}
    assert all(t.data_ptr() % 16 == 0 for t in out.values())          # the offsets of the case mean what the table says
    return out


def blank_destination(gpu, case):
    return upload(gpu, {w: K.blank(case, w) for w in K.PLANES[3:]})


ARGS = ("srcY", "srcU", "srcV", "src_strideY", "src_strideUV", "src_pitchY", "src_pitchUV", "num_pictures", "top", "bottom", "nv12", "bits",
        "width", "height", "dstY", "dstU", "dstV", "strideY", "strideUV", "pitchY", "pitchUV", "nframes")


def arguments(case, dsrc, ddst, top, bottom, nframes):
    """the C ABI's arguments for a case, by name (the refusal test changes one at a time)"""
    L = {w: K.plane(case, w) for w in K.planes_of(case)}
    a = {w: (dsrc if w in dsrc else ddst)[w].data_ptr() + L[w].base for w in L}
    a.setdefault("srcV", None)
    a.update(src_strideY=L["srcY"].stride, src_strideUV=L["srcU"].stride, src_pitchY=case.src_pitch[0], src_pitchUV=case.src_pitch[1],
             num_pictures=K.P, top=top, bottom=bottom, nv12=int(case.nv12), bits=case.bits, width=case.W, height=case.H,
             strideY=L["dstY"].stride, strideUV=L["dstU"].stride, pitchY=case.dst_pitch[0], pitchUV=case.dst_pitch[1], nframes=nframes)
    return a


def raw_weave(ctx, a, msb, handle="ctx"):
    """(return value, message) of one call"""
    ints = lambda v: None if v is None else (C.c_int * len(v))(*v)
    fn = ctx.lib.amtgpu_weave_fields_batch_msb if msb else ctx.lib.amtgpu_weave_fields_batch
    h = ctx.h if handle == "ctx" else None
    r = fn(h, *[ints(a[k]) if k in ("top", "bottom") else a[k] for k in ARGS])
    return r, ctx.lib.amtgpu_last_error(h).decode(errors="replace")


def assert_buffers(gpu, got, want, what):
    gpu["torch"].cuda.synchronize()
    for w in want:
        diff = K.first_difference(got[w].cpu().numpy(), want[w])
        assert not diff, f"{what}, {w}: {diff}"


@pytest.mark.parametrize("case", K.WEAVE_CASES, ids=lambda c: c.name)
def test_every_byte_of_the_destination(gpu, case):
    src = K.weave_source(case)
    dsrc = upload(gpu, src)
    # 6 frames from 5 pictures by the index arrays; then the identity (NULL arrays) for 5 frames, the sixth staying as it was
    for top, bottom, n in ((K.TOP, K.BOTTOM, K.N), (None, None, K.P)):
        ddst = blank_destination(gpu, case)
        r, msg = raw_weave(gpu["ctx"], arguments(case, dsrc, ddst, top, bottom, n), case.msb)
        assert r == 1, msg
        assert_buffers(gpu, ddst, K.weave_expected(case, src, top, bottom, n), "identity" if top is None else "indexed")
    assert_buffers(gpu, dsrc, src, "sources")


@pytest.mark.parametrize("top,bottom", [(None, K.BOTTOM), (K.TOP, None)], ids=["top-null", "bottom-null"])
def test_one_index_array_null(gpu, top, bottom):
    case = BY_NAME["02-vec-tails"]
    src = K.weave_source(case)
    dsrc, ddst = upload(gpu, src), blank_destination(gpu, case)
    r, msg = raw_weave(gpu["ctx"], arguments(case, dsrc, ddst, top, bottom, K.P), case.msb)
    assert r == 1, msg
    assert_buffers(gpu, ddst, K.weave_expected(case, src, top, bottom, K.P), "one array NULL")


def test_refusals_launch_nothing(gpu):
    """every throw of weave_fields(): 0, a message that names the reason, the whole destination still at its sentinel"""
    plain, nv12, msb = BY_NAME["01-vec-whole"], BY_NAME["10-nv12-two-split-rounds"], BY_NAME["13-elem-10bit-msb"]
    W, H = plain.W, plain.H
    at = lambda k, v: (K.TOP[:k] + (v,) + K.TOP[k + 1:])
    cases = [
        ("no context", plain, {}, "no context"),
        ("width 0", plain, dict(width=0), "width"),
        ("odd width", plain, dict(width=W - 1), "width"),
        ("height 0", plain, dict(height=0), "height"),
        ("height not a multiple of 4", plain, dict(height=H - 2), "height"),
        ("7 bits", plain, dict(bits=7), "bit depth"),
        ("17 bits", msb, dict(bits=17), "bit depth"),
        ("MSB at 8 bits", plain, dict(msb=True), "9..16"),
        ("null source Y", plain, dict(srcY=None), "null plane"),
        ("null source U", plain, dict(srcU=None), "null plane"),
        ("null source V", plain, dict(srcV=None), "null plane"),
        ("null interleaved plane", nv12, dict(srcU=None), "null plane"),
        ("null destination Y", plain, dict(dstY=None), "null plane"),
        ("null destination U", plain, dict(dstU=None), "null plane"),
        ("null destination V", plain, dict(dstV=None), "null plane"),
        ("source pitch below the luma row", plain, dict(src_pitchY=W - 1), "pitch"),
        ("source pitch below the chroma row", plain, dict(src_pitchUV=W // 2 - 1), "pitch"),
        ("interleaved pitch below both chroma rows", nv12, dict(src_pitchUV=nv12.W - 1), "pitch"),
        ("destination pitch below the luma row", plain, dict(pitchY=W - 1), "pitch"),
        ("destination pitch below the chroma row", plain, dict(pitchUV=W // 2 - 1), "pitch"),
        ("top -1", plain, dict(top=at(3, -1)), "index"),
        ("top past the last picture", plain, dict(top=at(5, K.P)), "index"),
        ("bottom -1", plain, dict(bottom=at(0, -1)), "index"),
        ("bottom past the last picture", plain, dict(bottom=at(2, K.P)), "index"),
        ("identity past the last picture", plain, dict(top=None, bottom=None), "index"),
        ("identity top past the last picture", plain, dict(top=None), "index"),
        ("identity bottom past the last picture", plain, dict(bottom=None), "index"),
        ("MSB: odd source Y", msb, dict(srcY=+1), "container size"),
        ("MSB: odd source Y stride", msb, dict(src_strideY=+1), "container size"),
        ("MSB: odd source U", msb, dict(srcU=+1), "container size"),
        ("MSB: odd source chroma stride", msb, dict(src_strideUV=+1), "container size"),
        ("MSB: odd source V", msb, dict(srcV=+1), "container size"),
        ("MSB: odd destination Y", msb, dict(dstY=+1), "container size"),
        ("MSB: odd destination Y stride", msb, dict(strideY=+1), "container size"),
        ("MSB: odd destination U", msb, dict(dstU=+1), "container size"),
        ("MSB: odd destination chroma stride", msb, dict(strideUV=+1), "container size"),
        ("MSB: odd destination V", msb, dict(dstV=+1), "container size"),
    ]
    ctx = gpu["ctx"]
    state = {}
    for case in (plain, nv12, msb):
        state[case.name] = (upload(gpu, K.weave_source(case)), blank_destination(gpu, case),
                            {w: K.blank(case, w) for w in K.PLANES[3:]})
    for what, case, change, reason in cases:
        dsrc, ddst, untouched = state[case.name]
        a = arguments(case, dsrc, ddst, K.TOP, K.BOTTOM, K.N)
        use_msb = change.pop("msb", case.msb)
        for k, v in change.items():
            a[k] = a[k] + v if what.startswith("MSB: odd") else v
        r, msg = raw_weave(ctx, a, use_msb, handle="none" if what == "no context" else "ctx")
        assert r == 0 and reason in msg, (what, r, msg)
        assert_buffers(gpu, ddst, untouched, what)
    # nothing to do is no refusal
    dsrc, ddst, untouched = state[plain.name]
    assert raw_weave(ctx, arguments(plain, dsrc, ddst, K.TOP, K.BOTTOM, 0), False)[0] == 1
    assert_buffers(gpu, ddst, untouched, "nframes == 0")
    # and the context is still good for a weave
    r, msg = raw_weave(ctx, arguments(plain, dsrc, ddst, K.TOP, K.BOTTOM, K.N), False)
    assert r == 1, msg
    assert_buffers(gpu, ddst, K.weave_expected(plain, K.weave_source(plain), K.TOP, K.BOTTOM, K.N), "after the refusals")
