"""csrc/resample.hip against Pillow, byte for byte: one ragged batch of images with zero, one and two BOX levels, widths whose rows
are no multiple of 4 bytes, an image larger than a workgroup tile in both directions; the regions the launches may write; the
single passes against the numpy executor; the refusals of the C entry."""
import numpy as np
import pytest
import torch

from resample_cases import BATCH16, TRANSFORMS, image, pillow

pytestmark = pytest.mark.gpu
R = 16
FILL = 0xA5


def _images():
    return [np.array(image(w, h)) for w, h in BATCH16]


@pytest.mark.parametrize("transform", TRANSFORMS)
def test_mixed_batch_equals_pillow_and_writes_only_its_regions(dev, transform):
    from reed_amd import resample
    assert any((3 * w) % 4 for w, _ in BATCH16)
    imgs = _images()
    plans = [resample.plan(im.shape[0], im.shape[1], transform, R) for im in imgs]
    if transform == "center-crop-dhariwal":
        assert {sum(p.axis == 1 for p in ps) for ps in plans} >= {0, 1, 2, 3}       # no pass, BICUBIC only, one and two BOX levels
    bp = resample.BatchPlan(plans, R)
    pad = 4096                                                                       # the tails of the arenas stay untouched too
    scratch = [torch.full((n + pad,), FILL, dtype=torch.uint8, device=dev) for n in bp.scratch_bytes]
    out = torch.full((bp.out_bytes + pad,), FILL, dtype=torch.uint8, device=dev)
    got = resample.center_crop_batch(imgs, transform, R, device=dev, plans=plans, out=out, scratch=scratch)
    torch.cuda.synchronize()
    assert got.shape == (len(imgs), 3, R, R) and got.dtype == torch.uint8 and got.data_ptr() == out.data_ptr()
    want = np.stack([pillow(w, h, transform, R) for w, h in BATCH16]).transpose(0, 3, 1, 2)
    bad = [BATCH16[i] for i in range(len(imgs)) if not np.array_equal(got[i].cpu().numpy(), want[i])]
    assert not bad, f"images that differ from Pillow: {bad}"
    # every byte outside the windows of the passes still holds the fill: pitch padding, untouched columns, the arenas' tails
    assert np.all(out.cpu().numpy()[bp.out_bytes:] == FILL)
    for par in (0, 1):
        mask = np.zeros(scratch[par].numel(), bool)
        for lev, (items, _) in enumerate(bp.levels):
            if lev % 2 == par:
                mask |= resample.written_mask(items, mask.size, planar=False)
        assert (mask.sum() > 0) == (bp.scratch_bytes[par] > 0) and mask.sum() < mask.size   # center-crop never uses the second arena
        assert np.all(scratch[par].cpu().numpy()[~mask] == FILL), f"scratch arena {par}: a byte outside the passes' windows was written"


@pytest.mark.parametrize("transform", TRANSFORMS)
def test_batch_of_one_gives_the_same_bytes(dev, transform):
    from reed_amd import resample
    imgs = _images()
    whole = resample.center_crop_batch(imgs, transform, R, device=dev).cpu()
    for i, im in enumerate(imgs):
        one = resample.center_crop_batch([im], transform, R, device=dev).cpu()
        assert one.shape == (1, 3, R, R) and torch.equal(one[0], whole[i]), BATCH16[i]


def _launch_one(dev, p, src_img):
    """A direct ops.resample_u8 call for the single pass p on src_img u8 [rows, columns, 3]; returns the destination arena (interleaved,
    pitch rounded up to 16 bytes, pre-filled) or the planar output."""
    from reed_amd import ops, resample
    h, w = p.src_shape
    sp, dp = resample.pitch_of(w), resample.pitch_of(p.dst_shape[1])
    arena = np.zeros((h, sp), np.uint8)
    arena[:, :3 * w] = src_img.reshape(h, 3 * w)
    kind = resample.KIND_H if p.axis == 1 else (resample.KIND_V_PLANAR if p.planar else resample.KIND_V)
    it = np.zeros(resample.ITEM_INTS, np.int32)
    it[4:] = [sp, p.noth if p.planar else dp, p.src_shape[p.axis], p.out0, p.nout, p.oth0, p.noth, 0, 0, p.coefs.shape[1], kind,
              p.nout * p.noth]
    tiles = -(-resample.item_units(kind, p.out0, p.nout, p.oth0, p.noth) // resample.TILE)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in dict(src=arena, items=it, prefix=np.array([0, tiles], np.int32),
                                                                              coefs=p.coefs, bounds=p.bounds).items()}
    dst = torch.full((p.dst_shape[0] * dp,), FILL, dtype=torch.uint8, device=dev)
    out = torch.full((3 * p.nout * p.noth,), FILL, dtype=torch.uint8, device=dev)
    ops.resample_u8(t["src"], dst, out, t["items"], t["prefix"], 1, tiles, t["coefs"], t["bounds"])
    torch.cuda.synchronize()
    return (out if p.planar else dst).cpu().numpy(), dp


@pytest.mark.parametrize("axis", [1, 0])
def test_single_pass_equals_the_numpy_executor(dev, axis):
    """The BICUBIC horizontal pass (a window that starts at column 3) and the BOX vertical pass of 53 x 37 -> R = 16, each alone,
    interleaved output."""
    from reed_amd import resample
    w, h = 53, 37
    passes = resample.plan(h, w, "center-crop-dhariwal", R)
    assert [(p.axis, p.planar) for p in passes] == [(1, False), (0, False), (1, False), (0, True)] and passes[2].out0 % 4
    cur = np.array(image(w, h))
    idx = [i for i, p in enumerate(passes) if p.axis == axis and not p.planar][-1]
    for p in passes[:idx]:
        cur = resample.execute_pass(cur, p)
    p = passes[idx]
    assert not p.planar
    want = resample.execute_pass(cur, p)
    got, dp = _launch_one(dev, p, cur)
    got = got.reshape(p.dst_shape[0], dp)
    rows = slice(p.out0, p.out0 + p.nout) if axis == 0 else slice(p.oth0, p.oth0 + p.noth)
    cols = slice(p.oth0, p.oth0 + p.noth) if axis == 0 else slice(p.out0, p.out0 + p.nout)
    inside = np.zeros(got.shape, bool)
    inside[rows, 3 * cols.start:3 * cols.stop] = True
    assert np.array_equal(got[rows, 3 * cols.start:3 * cols.stop], want[rows, cols].reshape(rows.stop - rows.start, -1))
    assert np.all(got[~inside] == FILL)


def test_entry_refuses_bad_arguments_without_a_launch(dev):
    from reed_amd import _lib
    L = _lib.load("bf16")
    buf = torch.full((4096,), FILL, dtype=torch.uint8, device=dev)
    tab = torch.zeros(64, dtype=torch.int32, device=dev)
    p, q = buf.data_ptr(), tab.data_ptr()
    ok = (p, p + 1024, p + 2048, q, q + 128, 1, 1, q + 64, q + 192, None)
    for i, v in [(5, 0), (5, -3), (6, 0), (0, None), (3, None), (4, None), (7, None), (8, None)]:
        args = list(ok)
        args[i] = v
        assert L.reed_resample_u8(*args) == 1001, (i, v)
        assert b"resample_u8" in L.reed_last_error()
    args = list(ok)
    args[1] = args[2] = None
    assert L.reed_resample_u8(*args) == 1001
    torch.cuda.synchronize()
    assert torch.all(buf == FILL)
