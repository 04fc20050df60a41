"""`python -m reed_amd.dataset convert` end to end: raw images of mixed sizes and formats -> the reference's image folder, the same
bytes through the HIP kernel and through Pillow, and the fused SD-VAE encode equal to convert followed by `dataset encode`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from resample_cases import image
from test_vae_encoder_gpu import _random_encoder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 32


def _run(args, timeout):
    r = subprocess.run([sys.executable, "-m", "reed_amd.dataset"] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _tree(root):
    return {os.path.relpath(os.path.join(r, f), root): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(root) for f in fs}


def _source(src):
    """Two class directories, seven images of different sizes (PNG, one JPEG, one grayscale, one smaller than R), a stray file."""
    import PIL.Image
    sizes = [(70, 45), (33, 64), (129, 131), (32, 32), (20, 27), (100, 40), (65, 97)]
    for i, (w, h) in enumerate(sizes):
        d = src / ("cats" if i < 3 else "dogs")
        d.mkdir(parents=True, exist_ok=True)
        pil = PIL.Image.fromarray(np.array(image(w, h)))
        if i == 1:
            pil.save(d / f"im{i}.jpg", quality=90)
        elif i == 5:
            pil.convert("L").save(d / f"im{i}.png")
        else:
            pil.save(d / f"im{i}.png")
    (src / "cats" / "readme.txt").write_text("not an image")
    return [0, 0, 0, 1, 1, 1, 1]


def test_convert_gpu_equals_pil_and_feeds_the_dataset(dev, tmp_path):
    import PIL.Image
    from safetensors.torch import save_file
    from reed_amd import resample
    from reed_amd.dataset import CustomDataset, list_image_folder
    src = tmp_path / "raw"
    labels = _source(src)
    enc = _random_encoder({}, 7, 0.02)
    ck = tmp_path / "sd-vae"
    ck.mkdir()
    save_file({k: v.contiguous() for k, v in enc.state_dict().items()}, str(ck / "diffusion_pytorch_model.safetensors"))
    data = tmp_path / "data"
    # the GPU path with the fused encode, batches of 3 (the last one ragged); the Pillow path alone
    _run(["convert", str(src), str(data / "images"), "--resolution", str(R), "--resize", "gpu", "--batch-size", "3", "--num-workers", "2",
          "--vae-sd-dest", str(data / "vae-sd"), "--vae-ckpt", str(ck)], timeout=600)
    _run(["convert", str(src), str(tmp_path / "pil"), "--resolution", str(R), "--resize", "pil", "--num-workers", "2"], timeout=600)
    got, want = _tree(data / "images"), _tree(tmp_path / "pil")
    names = ["00000/img%08d.png" % i for i in range(7)]
    assert sorted(got) == sorted(names + ["dataset.json"])
    assert got == want                                                   # byte-identical trees
    assert json.loads(got["dataset.json"]) == {"labels": [[n, lab] for n, lab in zip(names, labels)]}
    for n, (path, _) in zip(names, list_image_folder(str(src))):
        assert len(got[n]) >= R * R * 3                                  # uncompressed
        raw = np.array(PIL.Image.open(path).convert("RGB"))
        assert np.array_equal(np.array(PIL.Image.open(data / "images" / n)), resample.pil_transform(raw, "center-crop-dhariwal", R))
    # the fused moments: what `dataset encode` writes from the converted folder, byte for byte
    _run(["encode", str(data / "images"), str(tmp_path / "vae-sd-two-step"), "--vae-ckpt", str(ck), "--precision", "fp32",
          "--num-workers", "2"], timeout=600)
    fused, two = _tree(data / "vae-sd"), _tree(tmp_path / "vae-sd-two-step")
    assert sorted(fused) == ["00000/img-mean-std-%08d.npy" % i for i in range(7)] + ["dataset.json"]
    assert fused == two
    ds = CustomDataset(str(data))
    assert len(ds) == 7
    for i in range(7):
        img, moments, label, _ = ds[i]
        assert img.shape == (3, R, R) and img.dtype == torch.uint8 and moments.shape == (8, R // 8, R // 8) and int(label) == labels[i]
    # the other transform, and a second run into the now non-empty destination
    from reed_amd import dataset
    for how in ("gpu", "pil"):                                           # in this process: the subprocess plumbing is covered above
        dataset.main(["convert", str(src), str(tmp_path / f"cc-{how}"), "--resolution", str(R), "--transform", "center-crop",
                      "--resize", how, "--num-workers", "0"])
    assert _tree(tmp_path / "cc-gpu") == _tree(tmp_path / "cc-pil")
    r = subprocess.run([sys.executable, "-m", "reed_amd.dataset", "convert", str(src), str(data / "images"), "--resolution", str(R)],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "must be empty" in r.stderr
