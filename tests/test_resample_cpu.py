"""The host planner of `dataset convert` (reed_amd/resample.py) against Pillow: the coefficient tables and windows of every pass,
run by the numpy integer executor, give Pillow's bytes; and the refusals of convert's argument checks.  No GPU."""
import numpy as np
import pytest

from resample_cases import BATCH16, CASES, TRANSFORMS, image, pillow


@pytest.mark.parametrize("transform", TRANSFORMS)
@pytest.mark.parametrize("R,w,h", CASES + [(16, 520, 260)])
def test_plan_equals_pillow(R, w, h, transform):
    from reed_amd import resample
    passes = resample.plan(h, w, transform, R)
    got = resample.execute_plan(np.array(image(w, h)), passes)
    assert got.shape == (R, R, 3) and got.dtype == np.uint8
    assert np.array_equal(got, pillow(w, h, transform, R))


def test_both_clip_ends_fire():
    """About half of the images are thresholded to 0 / 255; on them the accumulators of the BICUBIC and of the LANCZOS passes
    leave [0, 255] at both ends, so the clip is part of what the comparisons with Pillow check."""
    from reed_amd import resample
    hard = [(R, w, h) for R, w, h in CASES if set(np.unique(image(w, h))) <= {0, 255}]
    assert len(CASES) // 2 - 1 <= len(hard) <= len(CASES) // 2 + 1
    for transform in TRANSFORMS:
        lo, hi = 0, 255
        for R, w, h in hard:
            cur = np.array(image(w, h))
            for p in resample.plan(h, w, transform, R):
                for i in range(p.nout):
                    s0, n = p.bounds[i]
                    seg = cur[s0:s0 + n, p.oth0:p.oth0 + p.noth] if p.axis == 0 else cur[p.oth0:p.oth0 + p.noth, s0:s0 + n].transpose(1, 0, 2)
                    v = ((seg.astype(np.int64) * p.coefs[i, :n].astype(np.int64)[:, None, None]).sum(0) + (1 << 21)) >> 22
                    lo, hi = min(lo, int(v.min())), max(hi, int(v.max()))
                cur = resample.execute_pass(cur, p)
        assert lo < 0 and hi > 255, (transform, lo, hi)


@pytest.mark.parametrize("transform", TRANSFORMS)
@pytest.mark.parametrize("R,w,h", CASES + [(256, 4000, 3000), (16, 16, 4001)])
def test_plan_windows_stay_inside_extents(R, w, h, transform):
    from reed_amd import resample
    passes = resample.plan(h, w, transform, R)
    assert passes[0].src_shape == (h, w)
    assert passes[-1].axis == 0 and passes[-1].planar and (passes[-1].nout, passes[-1].noth) == (R, R)
    for p, nxt in zip(passes, passes[1:] + [None]):
        first, taps = p.bounds[:, 0].astype(np.int64), p.bounds[:, 1].astype(np.int64)
        assert p.bounds.shape == (p.nout, 2) and p.coefs.shape[0] == p.nout and p.coefs.dtype == np.int32
        assert first.min() >= 0 and taps.min() >= 1 and taps.max() <= p.coefs.shape[1]
        assert (first + taps).max() <= p.src_shape[p.axis]
        assert 0 <= p.out0 and p.out0 + p.nout <= p.dst_shape[p.axis]
        assert 0 <= p.oth0 and p.oth0 + p.noth <= p.src_shape[1 - p.axis] == p.dst_shape[1 - p.axis]
        if nxt is not None:
            assert nxt.src_shape == p.dst_shape and not p.planar
            # the next pass reads only what this one computes
            lo, hi = int(nxt.bounds[:, 0].min()), int((nxt.bounds[:, 0] + nxt.bounds[:, 1]).max())
            rows = (p.out0, p.out0 + p.nout) if p.axis == 0 else (p.oth0, p.oth0 + p.noth)
            cols = (p.oth0, p.oth0 + p.noth) if p.axis == 0 else (p.out0, p.out0 + p.nout)
            need_rows = (lo, hi) if nxt.axis == 0 else (nxt.oth0, nxt.oth0 + nxt.noth)
            need_cols = (nxt.oth0, nxt.oth0 + nxt.noth) if nxt.axis == 0 else (lo, hi)
            assert rows[0] <= need_rows[0] and need_rows[1] <= rows[1] and cols[0] <= need_cols[0] and need_cols[1] <= cols[1]


def test_lanczos_tap_count_of_a_large_reduction():
    from reed_amd import resample
    bounds, coefs = resample.coefficients(4000, 256, "lanczos")
    assert 90 <= bounds[:, 1].max() <= coefs.shape[1] <= 100


def test_batch_plan_tables():
    """The device tables of a ragged batch: images without a pass at a level are absent from it, offsets and pitches are 16-byte
    multiples, the prefix counts the tiles, and every image ends in exactly one planar item at its own slot of the output."""
    from reed_amd import resample
    R = 16
    plans = [resample.plan(h, w, "center-crop-dhariwal", R) for w, h in BATCH16]
    assert {len(p) for p in plans} >= {1, 2, 4, 6, 8}            # zero, one and two BOX levels (and the plain copy) share launches
    bp = resample.BatchPlan(plans, R)
    assert len(bp.levels) == max(len(p) for p in plans)
    planar = []
    for lev, (items, prefix) in enumerate(bp.levels):
        assert items.shape == (sum(len(p) > lev for p in plans), resample.ITEM_INTS) and items.dtype == np.int32
        assert prefix.shape == (items.shape[0] + 1,) and prefix[0] == 0 and np.all(np.diff(prefix) >= 1)
        for it, tiles in zip(items, np.diff(prefix)):
            offs = it[0:4].view(np.int64)
            units = resample.item_units(int(it[14]), int(it[7]), int(it[8]), int(it[9]), int(it[10]))
            assert tiles == -(-units // resample.TILE)
            assert offs[0] % 16 == 0 and it[4] % 16 == 0
            if it[14] == resample.KIND_V_PLANAR:
                planar.append(int(offs[1]))
                assert it[5] == R and it[15] == R * R
            else:
                assert offs[1] % 16 == 0 and it[5] % 16 == 0
                assert offs[1] + int(it[5]) * (int(it[7]) + int(it[8]) if it[14] == resample.KIND_V else int(it[9]) + int(it[10])) \
                    <= bp.scratch_bytes[lev % 2]
    assert sorted(planar) == [b * 3 * R * R for b in range(len(plans))]


@pytest.mark.parametrize("bad,word", [(dict(transform="center-crop-wide"), "center-crop-wide"), (dict(resolution=48), "power-of-two"),
                                      (dict(resolution=4), "power-of-two"), (dict(source="zip"), "zip sources"),
                                      (dict(dest="zip"), "zip destinations"), (dict(dest="full"), "must be empty")])
def test_convert_refusals(tmp_path, bad, word):
    from reed_amd import dataset
    src, full = tmp_path / "src", tmp_path / "full"
    src.mkdir()
    full.mkdir()
    (full / "x.png").write_bytes(b"")
    (tmp_path / "a.zip").write_bytes(b"")
    source = str(tmp_path / "a.zip") if bad.get("source") == "zip" else str(src)
    dest = {"zip": str(tmp_path / "out.zip"), "full": str(full)}.get(bad.get("dest"), str(tmp_path / "out"))
    argv = ["convert", source, dest, "--resolution", str(bad.get("resolution", 32)), "--resize", "pil", "--num-workers", "0",
            "--transform", bad.get("transform", "center-crop-dhariwal")]
    with pytest.raises(SystemExit) as e:
        dataset.main(argv)
    assert "dataset convert:" in str(e.value) and word in str(e.value)
    with pytest.raises(ValueError):
        dataset.check_convert_args(source, dest, bad.get("resolution", 32), bad.get("transform", "center-crop-dhariwal"))


def test_convert_pil_path_writes_the_reference_layout(tmp_path):
    """`--resize pil` needs no GPU: file names, uncompressed PNGs holding Pillow's pixels, labels from the directory names."""
    import json
    import PIL.Image
    from reed_amd import dataset
    src = tmp_path / "src"
    sizes = [(37, 53), (64, 65), (20, 31)]
    for i, (w, h) in enumerate(sizes):
        d = src / ("b" if i else "a")
        d.mkdir(parents=True, exist_ok=True)
        PIL.Image.fromarray(np.array(image(w, h))).save(d / f"{i}.png")
    (src / "a" / "notes.txt").write_text("not an image")
    dataset.main(["convert", str(src), str(tmp_path / "images"), "--resolution", "16", "--resize", "pil", "--num-workers", "0",
                  "--batch-size", "2"])
    names = ["00000/img%08d.png" % i for i in range(3)]
    assert json.load(open(tmp_path / "images" / "dataset.json")) == {"labels": [[n, lab] for n, lab in zip(names, [0, 1, 1])]}
    for n, (w, h) in zip(names, sizes):
        f = tmp_path / "images" / n
        assert f.stat().st_size >= 16 * 16 * 3
        assert np.array_equal(np.array(PIL.Image.open(f)), pillow(w, h, "center-crop-dhariwal", 16))
