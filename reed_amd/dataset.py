"""CustomDataset — the reference's on-disk training format (image/dataset.py:18-85, written by
image/preprocessing/dataset_tools.py): <data>/images/**.png (uint8 RGB 256x256), <data>/vae-sd/**.npy (SD-VAE
moments f32 [8,32,32]) + vae-sd/dataset.json {"labels": [[fname, int], ...]}, optional <data>/<text_embeds_dir>/**.npy.
Item: (image u8[3,H,W], moments f32[8,h,w], label i64, text f32[Dt] or zeros_like(moments)).

Additive (not in the reference): `features_dirs=[...]` loads precomputed frozen-encoder patch features
<data>/<dir>/**.npy f32 [256, z] instead of running the encoder every step, and images are
optional when no on-the-fly encoder needs them.

`pack_dataset` / `PackedDataset`: at ~1000 images/s per GPU the reference format costs one PNG
decode and 2-3 small-file opens per image per step. Packing writes the same items, bit for bit and in the same
(sorted-filename) order, into one memory-mappable array per field; `PackedDataset[i]` returns exactly what
`CustomDataset[i]` returns.

`encode_image_folder` (`python -m reed_amd.dataset encode`) writes the vae-sd/ half of that format from an image folder: the
reference's `dataset_tools.py encode` for a directory source (same file names, same dataset.json, same f32 [8, H/8, W/8] moments),
with the SD-VAE encoder on this package's kernels (reed_amd/vae.py) instead of diffusers.

`convert_image_folder` (`python -m reed_amd.dataset convert`) writes the images/ half from raw images of any sizes: the reference's
`dataset_tools.py convert` for a directory source and destination (same file order, labels, file names, uncompressed PNGs with the
same bytes), with Pillow's crop / resize arithmetic on the GPU (reed_amd/resample.py, csrc/resample.hip) or through Pillow itself,
and optionally the vae-sd/ half from the same device batches.
"""
import json
import os

import numpy as np
import torch
from torch.utils.data import Dataset


class CustomDataset(Dataset):
    def __init__(self, data_dir, text_embeds_dir=None, features_dirs=None, need_images=True):
        self.images_dir = os.path.join(data_dir, "images")
        self.features_dir = os.path.join(data_dir, "vae-sd")
        self.need_images = need_images and os.path.isdir(self.images_dir)
        exts = {".png", ".jpg", ".jpeg", ".npy", ".bmp", ".webp"}

        def walk(root):
            return sorted(os.path.relpath(os.path.join(r, f), start=root) for r, _d, files in os.walk(root)
                          for f in files if os.path.splitext(f)[1].lower() in exts)

        self.image_fnames = walk(self.images_dir) if self.need_images else []
        self.feature_fnames = walk(self.features_dir)
        with open(os.path.join(self.features_dir, "dataset.json"), "rb") as f:
            labels = dict(json.load(f)["labels"])
        labels = np.array([labels[fn.replace("\\", "/")] for fn in self.feature_fnames])
        self.labels = labels.astype({1: np.int64, 2: np.float32}[labels.ndim])
        self.text_embeds_dir = text_embeds_dir
        if text_embeds_dir is not None:
            self.full_text_embeds_dir = os.path.join(data_dir, text_embeds_dir)
            assert os.path.exists(self.full_text_embeds_dir), f"Text embeds dir {self.full_text_embeds_dir} does not exist"
        self.z_dirs = [os.path.join(data_dir, d) for d in (features_dirs or [])]

    def __len__(self):
        if self.need_images:
            assert len(self.image_fnames) == len(self.feature_fnames), \
                "Number of feature files and label files should be same"
        return len(self.feature_fnames)

    @staticmethod
    def _stem(feature_fname):
        d, f = os.path.split(feature_fname)
        return os.path.join(d, os.path.splitext(f)[0].replace("img-mean-std-", "img"))

    def __getitem__(self, idx):
        ffn = self.feature_fnames[idx]
        features = np.load(os.path.join(self.features_dir, ffn))
        if self.need_images:
            ifn = self.image_fnames[idx]
            ext = os.path.splitext(ifn)[1].lower()
            if ext == ".npy":
                image = np.load(os.path.join(self.images_dir, ifn))
                image = image.reshape(-1, *image.shape[-2:])
            else:
                import PIL.Image
                image = np.array(PIL.Image.open(os.path.join(self.images_dir, ifn)))
                image = image.reshape(*image.shape[:2], -1).transpose(2, 0, 1)
            image = torch.from_numpy(image)
            stem = os.path.splitext(ifn)[0]
        else:
            image = torch.zeros(0, dtype=torch.uint8)
            stem = self._stem(ffn)
        if self.text_embeds_dir is not None:
            text = torch.from_numpy(np.load(os.path.join(self.full_text_embeds_dir, stem + ".npy")))
        else:
            text = torch.zeros_like(torch.from_numpy(features))
        out = (image, torch.from_numpy(features), torch.tensor(self.labels[idx]), text)
        if self.z_dirs:
            out = out + tuple(torch.from_numpy(np.load(os.path.join(d, stem + ".npy"))).float() for d in self.z_dirs)
        return out


PACK_META = "packed.json"


def pack_dataset(data_dir, out_dir, text_embeds_dir=None, features_dirs=None, with_images=True, log_every=0):
    """Write <out_dir>/{moments,labels[,images][,text][,z0,z1,...]}.npy + packed.json from the reference format."""
    ds = CustomDataset(data_dir, text_embeds_dir=text_embeds_dir, features_dirs=features_dirs, need_images=with_images)
    n = len(ds)
    if n == 0:
        raise ValueError(f"{data_dir}: empty dataset")
    os.makedirs(out_dir, exist_ok=True)
    first = ds[0]
    fields = ["images", "moments", "labels", "text"] + [f"z{j}" for j in range(len(first) - 4)]
    keep = {"images": with_images and ds.need_images, "text": text_embeds_dir is not None}
    arrays = {}
    for name, t in zip(fields, first):
        if not keep.get(name, True):
            continue
        arrays[name] = np.lib.format.open_memmap(os.path.join(out_dir, name + ".npy"), mode="w+",
                                                 dtype=t.numpy().dtype, shape=(n,) + tuple(t.shape))
    for i in range(n):
        item = first if i == 0 else ds[i]
        for name, t in zip(fields, item):
            if name in arrays:
                if tuple(t.shape) != arrays[name].shape[1:]:
                    raise ValueError(f"item {i}: field {name} has shape {tuple(t.shape)}, expected {arrays[name].shape[1:]}")
                arrays[name][i] = t.numpy()
        if log_every and (i + 1) % log_every == 0:
            print(f"[pack_dataset] {i + 1}/{n}", flush=True)
    for a in arrays.values():
        a.flush()
    meta = {"n": n, "fields": {k: {"dtype": str(v.dtype), "shape": list(v.shape[1:])} for k, v in arrays.items()},
            "source": os.path.abspath(data_dir), "text_embeds_dir": text_embeds_dir, "features_dirs": features_dirs or []}
    with open(os.path.join(out_dir, PACK_META), "w") as f:
        json.dump(meta, f, indent=1)
    return meta


class PackedDataset(Dataset):
    """Items of `CustomDataset` from memory-mapped arrays (`pack_dataset`): same tuple, same dtypes, same order."""

    def __init__(self, packed_dir):
        with open(os.path.join(packed_dir, PACK_META)) as f:
            self.meta = json.load(f)
        self.n = self.meta["n"]
        self.arr = {k: np.load(os.path.join(packed_dir, k + ".npy"), mmap_mode="r") for k in self.meta["fields"]}
        self.zkeys = sorted((k for k in self.arr if k.startswith("z")), key=lambda k: int(k[1:]))

    def __len__(self):
        return self.n

    def _get(self, k, idx):
        return torch.from_numpy(np.array(self.arr[k][idx]))   # copy out of the mapping

    def __getitem__(self, idx):
        moments = self._get("moments", idx)
        image = self._get("images", idx) if "images" in self.arr else torch.zeros(0, dtype=torch.uint8)
        text = self._get("text", idx) if "text" in self.arr else torch.zeros_like(moments)
        out = (image, moments, torch.tensor(self.arr["labels"][idx]), text)
        return out + tuple(self._get(k, idx).float() for k in self.zkeys)


class SyntheticLatents(Dataset):
    """Random ImageNet-256-shaped items (SURVEY.md §8d synthetic inputs): for plumbing tests and throughput runs.  Latents and
    labels are drawn per index; the encoder features (1 MB per item for a 256 x 1024 target: drawing them per item costs 3 ms of
    host time, i.e. 300 items/s per loader process) come from a pool of `pool` tensors per encoder drawn once per process."""

    def __init__(self, n, z_dims=(), z_types=(), num_classes=1000, seed=0, latent=32, pool=32):
        self.n, self.z_dims, self.z_types, self.nc, self.seed, self.latent = n, list(z_dims), list(z_types), num_classes, seed, latent
        self.pool = max(1, int(pool))
        self._zs = None

    def __len__(self):
        return self.n

    def _pool(self):
        if self._zs is None:
            T = (self.latent // 2) ** 2
            g = torch.Generator().manual_seed(self.seed * 7919 + 17)
            self._zs = [torch.randn(self.pool, T, z, generator=g) if k == "i" else torch.randn(self.pool, z, generator=g)
                        for z, k in zip(self.z_dims, self.z_types)]
        return self._zs

    def __getitem__(self, idx):
        g = torch.Generator().manual_seed(self.seed * 1000003 + idx)
        mean = torch.randn(4, self.latent, self.latent, generator=g) * 5.49
        moments = torch.cat([mean, torch.full_like(mean, 0.5)], 0)
        label = torch.randint(0, self.nc, (), generator=g)
        zs = tuple(z[idx % self.pool] for z in self._pool())
        return (torch.zeros(0, dtype=torch.uint8), moments, label, torch.zeros(0)) + zs


# ---------------- dataset encode: image folder -> vae-sd moments ----------------
def _is_image(fname):
    import PIL.Image
    PIL.Image.init()
    return "." + fname.split(".")[-1].lower() in PIL.Image.EXTENSION


def list_image_folder(source_dir, max_images=None):
    """The images `dataset_tools.py encode` takes from a directory, in its order, with its labels (open_image_folder): every file
    under `source_dir` with an image extension, sorted by path; labels from <source_dir>/dataset.json {"labels": [[relpath,
    label], ...]}, or, when it has none, the index of the sorted top-level directory name when there is more than one.
    Returns [(path, label or None), ...] for the first `max_images`."""
    found = []
    for root, _dirs, files in os.walk(source_dir):
        found += [os.path.join(root, f) for f in files]
    paths = sorted(f for f in found if _is_image(f))
    rel = {f: os.path.relpath(f, source_dir).replace("\\", "/") for f in paths}
    labels = {}
    meta = os.path.join(source_dir, "dataset.json")
    if os.path.isfile(meta):
        with open(meta) as f:
            data = json.load(f)["labels"]
        if data is not None:
            labels = {x[0]: x[1] for x in data}
    if not labels:
        top = {r: r.split("/")[0] if "/" in r else "" for r in rel.values()}
        index = {name: i for i, name in enumerate(sorted(set(top.values())))}
        if len(index) > 1:
            labels = {r: index[name] for r, name in top.items()}
    n = len(paths) if max_images is None else min(len(paths), max_images)
    return [(f, labels.get(rel[f])) for f in paths[:n]]


def moments_fname(idx):
    s = f"{idx:08d}"
    return f"{s[:5]}/img-mean-std-{s}.npy"


def moments_metadata(items):
    """dataset.json of the encoded folder: {"labels": [[moments file, label], ...]}, or null when any image has no label."""
    labels = [[moments_fname(i), lab] if lab is not None else None for i, (_, lab) in enumerate(items)]
    return {"labels": labels if all(x is not None for x in labels) else None}


def _write_moments(dest_dir, idx, moments):
    """Save a batch of moments (f32 [B, 8, h, w], any device) as the files idx, idx + 1, ...; returns the next index."""
    for m in moments.cpu().numpy():
        fn = os.path.join(dest_dir, moments_fname(idx))
        os.makedirs(os.path.dirname(fn), exist_ok=True)
        np.save(fn, m)
        idx += 1
    return idx


def _write_metadata(dest_dir, meta):
    with open(os.path.join(dest_dir, "dataset.json"), "w") as f:
        f.write(json.dumps(meta))
    return meta


def _check_folders(source_dir, dest_dir):
    if not os.path.isdir(source_dir):
        raise ValueError(f"{source_dir}: not a directory (zip sources are not supported)")
    if dest_dir.lower().endswith(".zip"):
        raise ValueError(f"{dest_dir}: zip destinations are not supported")
    if os.path.isdir(dest_dir) and os.listdir(dest_dir):
        raise ValueError(f"{dest_dir}: the destination folder must be empty")


class _ImageFiles(Dataset):
    def __init__(self, paths):
        self.paths = paths

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        import PIL.Image
        img = np.array(PIL.Image.open(self.paths[i]).convert("RGB"))
        return torch.from_numpy(img).permute(2, 0, 1).contiguous(), self.paths[i]


def _collate_one_size(items):
    first = items[0]
    for img, path in items:
        if img.shape != first[0].shape:
            raise ValueError(f"{path} is {img.shape[2]}x{img.shape[1]} pixels but {first[1]} is {first[0].shape[2]}x{first[0].shape[1]}: "
                             "dataset encode needs images of one size (as `convert` writes them)")
    return torch.stack([img for img, _ in items]), [path for _, path in items]


def encode_image_folder(source_dir, dest_dir, vae_ckpt, precision="fp32", batch_size=8, max_images=None, num_workers=4,
                        device="cuda", log_every=0):
    """Write <dest_dir>/{00000/img-mean-std-00000000.npy, ...} (f32 [8, H/8, W/8] = cat[mean, std] of the SD-VAE posterior) and
    <dest_dir>/dataset.json for the images of `source_dir` (list_image_folder).  The files do not depend on `batch_size`."""
    _check_folders(source_dir, dest_dir)
    items = list_image_folder(source_dir, max_images)
    if not items:
        raise ValueError(f"{source_dir}: no images")
    from .vae import load_sd_vae_encoder
    vae = load_sd_vae_encoder(vae_ckpt, device=device)
    os.makedirs(dest_dir, exist_ok=True)
    loader = torch.utils.data.DataLoader(_ImageFiles([p for p, _ in items]), batch_size=batch_size, shuffle=False,
                                         num_workers=num_workers, pin_memory=True, collate_fn=_collate_one_size)
    idx, shape = 0, None
    for raw, paths in loader:
        if shape is None:
            shape, first = raw.shape[1:], paths[0]
        elif raw.shape[1:] != shape:
            raise ValueError(f"{paths[0]} is {raw.shape[3]}x{raw.shape[2]} pixels but {first} is {shape[2]}x{shape[1]}: "
                             "dataset encode needs images of one size (as `convert` writes them)")
        idx = _write_moments(dest_dir, idx, vae.encode(raw.to(device, non_blocking=True), precision=precision))
        if log_every and idx % log_every < len(paths):
            print(f"[dataset encode] {idx}/{len(items)}", flush=True)
    return _write_metadata(dest_dir, moments_metadata(items))


# ---------------- dataset convert: raw images -> images/ (and vae-sd/) ----------------
def image_fname(idx):
    s = f"{idx:08d}"
    return f"{s[:5]}/img{s}.png"


def image_metadata(items):
    """dataset.json of the converted folder: {"labels": [[image file, label], ...]}, or null when any image has no label."""
    labels = [[image_fname(i), lab] if lab is not None else None for i, (_, lab) in enumerate(items)]
    return {"labels": labels if all(x is not None for x in labels) else None}


def check_convert_args(source_dir, dest_dir, resolution, transform):
    """The refusals of `dataset convert`, each with its reason (ValueError)."""
    from .resample import TRANSFORMS
    _check_folders(source_dir, dest_dir)
    if transform == "center-crop-wide":
        raise ValueError("--transform center-crop-wide is not supported: its output is not square, and the dataset format needs "
                         "square images")
    if transform not in TRANSFORMS:
        raise ValueError(f"--transform {transform}: one of {', '.join(TRANSFORMS)}")
    if not isinstance(resolution, int) or resolution < 8 or resolution & (resolution - 1):
        raise ValueError(f"--resolution {resolution}: the dataset format needs square power-of-two images of at least 8 pixels")


class _RawImages(Dataset):
    """Decode (and, for `--resize pil`, crop and resize) in the loader's workers; no GPU is touched here.  The GPU path gets the
    decoded pixels and their plan of passes (the coefficient tables), so the main process only concatenates tables."""

    def __init__(self, paths, transform, resolution, resize):
        self.paths, self.transform, self.resolution, self.resize = paths, transform, resolution, resize

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        import PIL.Image
        from . import resample
        img = np.array(PIL.Image.open(self.paths[i]).convert("RGB"))
        if self.resize == "pil":   # tensors travel from the workers through shared memory, arrays through a pipe
            return torch.from_numpy(resample.pil_transform(img, self.transform, self.resolution)), None
        return torch.from_numpy(img), resample.plan(img.shape[0], img.shape[1], self.transform, self.resolution)


def _collate_list(items):
    return items


def convert_image_folder(source_dir, dest_dir, resolution, transform="center-crop-dhariwal", resize="pil", batch_size=64,
                         max_images=None, num_workers=4, vae_sd_dest=None, vae_ckpt=None, precision="fp32", device="cuda",
                         log_every=0):
    """Write <dest_dir>/{00000/img00000000.png, ...} (uncompressed RGB PNGs, resolution x resolution) and <dest_dir>/dataset.json
    for the images of `source_dir` (list_image_folder), cropped and resized as the reference's `convert --transform` does.
    resize "gpu": Pillow's arithmetic on the HIP kernel (resample.center_crop_batch); "pil": Pillow in the workers; the files are
    the same.  With `vae_sd_dest` and `vae_ckpt` every cropped batch also goes through the SD-VAE encoder and its moments are
    written as `encode_image_folder` would write them from <dest_dir>.  The files do not depend on `batch_size`."""
    import PIL.Image
    check_convert_args(source_dir, dest_dir, resolution, transform)
    if resize not in ("gpu", "pil"):
        raise ValueError(f"--resize {resize}: gpu or pil")
    if (vae_sd_dest is None) != (vae_ckpt is None):
        raise ValueError("--vae-sd-dest and --vae-ckpt go together")
    if vae_sd_dest is not None:
        _check_folders(source_dir, vae_sd_dest)
        if os.path.abspath(vae_sd_dest) == os.path.abspath(dest_dir):
            raise ValueError(f"{vae_sd_dest}: the moments need a folder of their own")
    items = list_image_folder(source_dir, max_images)
    if not items:
        raise ValueError(f"{source_dir}: no images")
    if (resize == "gpu" or vae_sd_dest is not None) and not torch.cuda.is_available():
        raise ValueError("no GPU: --resize gpu and --vae-sd-dest run on one (--resize pil needs none)")
    vae = None
    if vae_sd_dest is not None:
        from .vae import load_sd_vae_encoder
        vae = load_sd_vae_encoder(vae_ckpt, device=device)
        os.makedirs(vae_sd_dest, exist_ok=True)
    if resize == "gpu":
        from .resample import center_crop_batch
    os.makedirs(dest_dir, exist_ok=True)
    loader = torch.utils.data.DataLoader(_RawImages([p for p, _ in items], transform, resolution, resize), batch_size=batch_size,
                                         shuffle=False, num_workers=num_workers, collate_fn=_collate_list)
    idx = 0
    for batch in loader:
        if resize == "gpu":
            raw = center_crop_batch([im.numpy() for im, _ in batch], transform, resolution, device=device, plans=[p for _, p in batch])
            pixels = raw.permute(0, 2, 3, 1).cpu().numpy()
        else:
            pixels = torch.stack([im for im, _ in batch]).numpy()
            raw = torch.from_numpy(pixels).permute(0, 3, 1, 2).contiguous().to(device) if vae is not None else None
        if vae is not None:
            _write_moments(vae_sd_dest, idx, vae.encode(raw, precision=precision))
        for hwc in pixels:
            fn = os.path.join(dest_dir, image_fname(idx))
            os.makedirs(os.path.dirname(fn), exist_ok=True)
            PIL.Image.fromarray(np.ascontiguousarray(hwc)).save(fn, format="png", compress_level=0, optimize=False)
            idx += 1
        if log_every and idx % log_every < len(batch):
            print(f"[dataset convert] {idx}/{len(items)}", flush=True)
    if vae is not None:
        _write_metadata(vae_sd_dest, moments_metadata(items))
    return _write_metadata(dest_dir, image_metadata(items))


# the faster of the two end to end in profiles/dataset_convert.txt (382 against 310 images/s: the main process, which writes the
# PNGs, bounds both, and the GPU path gives it more to copy); the files are the same either way
CONVERT_RESIZE_DEFAULT = "pil"


def build_parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m reed_amd.dataset")
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("pack", help="pack <data_dir> into memory-mappable arrays (PackedDataset)")
    p.add_argument("data_dir")
    p.add_argument("out_dir")
    p.add_argument("--text-embeds-dir", default=None)
    p.add_argument("--features-dirs", nargs="*", default=None)
    p.add_argument("--no-images", action="store_true")
    e = sub.add_parser("encode", help="encode an image folder into SD-VAE moments (vae-sd/)",
                       description="Encode the images of a folder (e.g. the images/ output of the reference's `convert`) into the "
                                   "f32 [8, H/8, W/8] SD-VAE moments cat[mean, std] that `train --data-dir` reads, as the reference's "
                                   "`dataset_tools.py encode` does: <dest_dir>/00000/img-mean-std-00000000.npy, ... and dataset.json. "
                                   "Runs on the GPU. Directories only: zip sources and zip destinations are not supported. All "
                                   "images must have the same size; the destination must be empty or absent.")
    e.add_argument("source_images_dir")
    e.add_argument("dest_dir")
    e.add_argument("--vae-ckpt", required=True, help="sd-vae-ft-{mse,ema}: a diffusers directory, .safetensors or .bin")
    e.add_argument("--precision", choices=["fp32", "tf32", "fp16", "bf16"], default="fp32",
                   help="GEMM operand type (fp32: exact products; fp16 carries the mantissa of the reference's TF32 convolutions; tf32: "
                        "fp32 operands, activations and range with every product as three bf16 MFMA products, closer to fp32 than "
                        "TF32 and without fp16's channel-count rule)")
    e.add_argument("--batch-size", type=int, default=8, help="images per encoder call (the files do not depend on it)")
    e.add_argument("--max-images", type=int, default=None)
    e.add_argument("--num-workers", type=int, default=4, help="PNG decode processes (at most 16)")
    c = sub.add_parser("convert", help="crop and resize raw images into an image folder (images/), optionally with vae-sd/",
                       description="Crop and resize every image under a folder (any sizes, any format Pillow opens) to RxR and write "
                                   "them as the reference's `dataset_tools.py convert` does: <dest_images_dir>/00000/img00000000.png, "
                                   "... (uncompressed PNG) and dataset.json with labels from <source_dir>/dataset.json or the "
                                   "top-level directory names.  The pixels are Pillow's, bit for bit, on either --resize path. "
                                   "Directories only; the destination must be empty or absent.")
    c.add_argument("source_dir")
    c.add_argument("dest_images_dir")
    c.add_argument("--resolution", type=int, required=True, help="R: output is RxR, a power of two of at least 8")
    c.add_argument("--transform", default="center-crop-dhariwal",
                   help="center-crop-dhariwal (ADM's: BOX halvings, BICUBIC, centre crop; the default) or center-crop (crop, LANCZOS)")
    c.add_argument("--resize", choices=["gpu", "pil"], default=CONVERT_RESIZE_DEFAULT,
                   help="where the crop / resize runs: the HIP kernel, or Pillow in the workers (same files)")
    c.add_argument("--batch-size", type=int, default=64, help="images per launch (the files do not depend on it)")
    c.add_argument("--max-images", type=int, default=None)
    c.add_argument("--num-workers", type=int, default=4, help="decode processes (at most 16)")
    c.add_argument("--vae-sd-dest", default=None, help="also encode every cropped batch into SD-VAE moments here (needs --vae-ckpt)")
    c.add_argument("--vae-ckpt", default=None, help="sd-vae-ft-{mse,ema}: a diffusers directory, .safetensors or .bin")
    c.add_argument("--precision", choices=["fp32", "tf32", "fp16", "bf16"], default="fp32",
                   help="the encoder's GEMM operand type (tf32: as for `encode`)")
    return ap


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.cmd == "pack":
        m = pack_dataset(a.data_dir, a.out_dir, a.text_embeds_dir, a.features_dirs, with_images=not a.no_images, log_every=10000)
        print(json.dumps(m))
        return
    if a.batch_size < 1 or (a.max_images is not None and a.max_images < 1) or not 0 <= a.num_workers <= 16:
        ap.error("--batch-size and --max-images must be at least 1, --num-workers in [0, 16]")
    if a.cmd == "convert":
        try:
            meta = convert_image_folder(a.source_dir, a.dest_images_dir, a.resolution, transform=a.transform, resize=a.resize,
                                        batch_size=a.batch_size, max_images=a.max_images, num_workers=a.num_workers,
                                        vae_sd_dest=a.vae_sd_dest, vae_ckpt=a.vae_ckpt, precision=a.precision, log_every=10000)
        except ValueError as err:
            raise SystemExit(f"dataset convert: {err}")
        print(json.dumps({"dest": a.dest_images_dir, "vae_sd_dest": a.vae_sd_dest, "labelled": meta["labels"] is not None}))
        return
    try:
        meta = encode_image_folder(a.source_images_dir, a.dest_dir, a.vae_ckpt, precision=a.precision, batch_size=a.batch_size,
                                   max_images=a.max_images, num_workers=a.num_workers, log_every=10000)
    except ValueError as err:
        raise SystemExit(f"dataset encode: {err}")
    n = len(meta["labels"]) if meta["labels"] is not None else None
    print(json.dumps({"dest": a.dest_dir, "labelled": n is not None}))


if __name__ == "__main__":   # python -m reed_amd.dataset pack <data_dir> <out_dir> [--text-embeds-dir D] [--features-dirs A B] [--no-images]
    main()                   # python -m reed_amd.dataset encode <source_images_dir> <dest_dir> --vae-ckpt PATH [...]
                             # python -m reed_amd.dataset convert <source_dir> <dest_images_dir> --resolution R [...]
