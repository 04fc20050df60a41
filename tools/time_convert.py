"""`python -m reed_amd.dataset convert`: the two numbers of profiles/dataset_convert.txt.
  kernel      device time of all pass levels (csrc/resample.hip) for a batch of 500x375 images at R = 256, center-crop-dhariwal,
              against the bytes the passes read and write (computed from the plans' windows); device events around `reps`
              repetitions of the launches on staged tables, after a warm-up.  The result is checked against Pillow first.
  end to end  images/s of `convert --resize gpu` and of `convert --resize pil` on the same synthetic 500x375 JPEGs (written here from a
              seed), same process, same --num-workers, alternating, host clock around the whole call (the decode, the crop /
              resize, the PNG writes, dataset.json); one untimed run of each path first.
usage (GPU box): python tools/time_convert.py [--batch 64] [--reps 200] [--images 3000] [--workers 16] [--rounds 2] [--tmp DIR]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from reed_amd import dataset, resample  # noqa: E402

HBM_BYTES_PER_S = 8e12


def synthetic(rng, w=500, h=375):
    """A smooth random picture with some grain: JPEG-friendly, as photographs are"""
    import PIL.Image
    low = rng.integers(0, 256, (h // 25, w // 25, 3), dtype=np.uint8)
    img = np.array(PIL.Image.fromarray(low).resize((w, h), PIL.Image.Resampling.BICUBIC)).astype(np.int16)
    return np.clip(img + rng.integers(-12, 13, img.shape), 0, 255).astype(np.uint8)


def pass_bytes(plans):
    rd = wr = 0
    for ps in plans:
        for p in ps:
            span = int((p.bounds[:, 0] + p.bounds[:, 1]).max() - p.bounds[:, 0].min())
            rd += 3 * span * p.noth
            wr += 3 * p.nout * p.noth
    return rd, wr


def kernel_time(a, dev):
    rng = np.random.default_rng(0)
    R = 256
    imgs = [synthetic(rng) for _ in range(a.batch)]
    plans = [resample.plan(im.shape[0], im.shape[1], "center-crop-dhariwal", R) for im in imgs]
    got = resample.center_crop_batch(imgs, "center-crop-dhariwal", R, device=dev, plans=plans).cpu().numpy()
    want = np.stack([resample.pil_transform(im, "center-crop-dhariwal", R) for im in imgs]).transpose(0, 3, 1, 2)
    assert np.array_equal(got, want), "the kernel's bytes differ from Pillow's"
    bp = resample.BatchPlan(plans, R)
    scratch = [torch.empty(max(n, 16), dtype=torch.uint8, device=dev) for n in bp.scratch_bytes]
    out = torch.empty(bp.out_bytes, dtype=torch.uint8, device=dev)
    tables = resample.stage_batch(imgs, bp, dev)
    for _ in range(10):
        resample.run_levels(bp, tables, scratch, out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        resample.run_levels(bp, tables, scratch, out)
    e1.record()
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1) * 1e-3 / a.reps
    rd, wr = pass_bytes(plans)
    print(f"kernel: batch {a.batch} x 500x375 -> {R}^2, {len(bp.levels)} launches (levels) per batch, {a.reps} repetitions")
    print(f"  device time per batch {t * 1e6:.1f} us = {t * 1e6 / len(bp.levels):.1f} us per launch, {a.batch / t:.0f} images/s")
    print(f"  bytes the passes read {rd / 1e6:.2f} MB + write {wr / 1e6:.2f} MB = {(rd + wr) / t / 1e9:.1f} GB/s, "
          f"{(rd + wr) / t / HBM_BYTES_PER_S * 100:.2f} % of 8 TB/s")
    t0 = time.perf_counter()
    for _ in range(20):
        resample.BatchPlan(plans, R)
    print(f"  host: BatchPlan (concatenating the tables) {(time.perf_counter() - t0) / 20 * 1e3:.2f} ms per batch; "
          f"plan() {sum(_t_plan() for _ in range(20)) / 20 * 1e3:.2f} ms per image (in the workers)")


def _t_plan():
    t0 = time.perf_counter()
    resample.plan(375, 500, "center-crop-dhariwal", 256)
    return time.perf_counter() - t0


def end_to_end(a):
    import PIL.Image
    tmp = tempfile.mkdtemp(dir=a.tmp)
    try:
        rng = np.random.default_rng(1)
        src = os.path.join(tmp, "raw")
        t0 = time.perf_counter()
        for i in range(a.images):
            d = os.path.join(src, f"class{i % 10}")
            os.makedirs(d, exist_ok=True)
            PIL.Image.fromarray(synthetic(rng)).save(os.path.join(d, f"{i:06d}.jpg"), quality=90)
        print(f"end to end: {a.images} synthetic 500x375 JPEGs written in {time.perf_counter() - t0:.1f} s; --resolution 256, "
              f"--num-workers {a.workers}, --batch-size 64")

        def run(how, n):
            dest = os.path.join(tmp, "dest")
            t0 = time.perf_counter()
            dataset.convert_image_folder(src, dest, 256, resize=how, batch_size=64, max_images=n, num_workers=a.workers)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            shutil.rmtree(dest)
            return dt

        for how in ("gpu", "pil"):
            run(how, 256)
        rates = {"gpu": [], "pil": []}
        for _ in range(a.rounds):
            for how in ("gpu", "pil"):
                rates[how].append(a.images / run(how, None))
                print(f"  --resize {how}: {rates[how][-1]:8.1f} images/s", flush=True)
        for how in ("gpu", "pil"):
            print(f"  --resize {how}: best {max(rates[how]):.1f}, worst {min(rates[how]):.1f} images/s over {a.rounds} runs")
        # where the time goes on the CPU path: one process, no loader
        files = [p for p, _ in dataset.list_image_folder(src, 200)]
        t0 = time.perf_counter()
        raw = [np.array(PIL.Image.open(f).convert("RGB")) for f in files]
        t1 = time.perf_counter()
        for im in raw:
            resample.pil_transform(im, "center-crop-dhariwal", 256)
        t2 = time.perf_counter()
        print(f"  one CPU process, 200 images: decode {(t1 - t0) / 200 * 1e3:.2f} ms, Pillow crop / resize {(t2 - t1) / 200 * 1e3:.2f} ms "
              f"per image ({(t2 - t1) / (t2 - t0) * 100:.0f} % of the two)")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--images", type=int, default=3000)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--tmp", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    print(torch.cuda.get_device_name(0))
    kernel_time(a, dev)
    end_to_end(a)


if __name__ == "__main__":
    main()
