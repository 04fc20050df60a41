"""Pillow's 8-bit resampler (ImagingResample) as a plan of integer passes: the crop / resize of the reference's
`dataset_tools.py convert` (image/preprocessing/dataset_tools.py:131-200, make_transform), bit for bit.

`Image.resize` runs a horizontal pass, then a vertical one, each uint8 -> uint8 with 22-bit fixed-point coefficients.  `plan()`
rebuilds the coefficient tables on the host (numpy float64, no fused multiply-add, sequential sums) and trims every pass to the
window later passes read; `execute_plan()` runs a plan in numpy integers (the CPU oracle of the tables); `center_crop_batch()`
runs the plans of a ragged batch on the GPU (csrc/resample.hip through ops.resample_u8), one launch per pass level.

Geometry: a pass keeps the coordinates of its axes.  Its destination has the full extent of the resized image, and only the
window [out0, out0 + nout) x [oth0, oth0 + noth) of it is computed; a crop in front of a resize (`center-crop`) is a shift of the
taps' first sample.  The last pass of every plan is vertical and writes the R x R crop window (an image that needs no resampling
gets a one-tap identity pass), so its result is the planar u8 [3, R, R] the trainer and the SD-VAE encoder take.

This module imports no torch at import time: the planner runs in the DataLoader workers next to the JPEG decode.
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
TRANSFORMS = ("center-crop-dhariwal", "center-crop")
KIND_H, KIND_V, KIND_V_PLANAR = 0, 1, 2
ITEM_INTS = 16   # int32 words per item of the device table (include/reed_hip.h, reed_resample_u8)
ALIGN = 16       # row pitches and image offsets of the arenas, bytes


def _box(x):
    return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)


def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    out = np.zeros(x.shape, np.float64)
    flat, o = x.ravel(), out.ravel()
    for i in np.nonzero((flat >= -3.0) & (flat < 3.0))[0]:   # math.sin: the C library's, as Pillow calls it
        v = float(flat[i])
        o[i] = _sinc(v) * _sinc(v / 3)
    return out


FILTERS = {"box": (_box, 0.5), "bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


def coefficients(n_in, n_out, filt, o0=0, o1=None):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the outputs [o0, o1) of an axis resized from n_in to n_out samples:
    (bounds int32 [n, 2] = (first source sample, taps), coefs int32 [n, ksize])."""
    f, support = FILTERS[filt]
    o1 = n_out if o1 is None else o1
    scale = n_in / n_out
    fs = max(scale, 1.0)
    sup = support * fs
    ksize = int(math.ceil(sup)) * 2 + 1
    ss = 1.0 / fs
    xx = np.arange(o0, o1, dtype=np.float64)
    c = (xx + 0.5) * scale
    xmin = np.maximum(np.trunc(c - sup + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(c + sup + 0.5).astype(np.int64), n_in) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < xmax[:, None]
    w = np.where(live, f((x + xmin[:, None] - c[:, None] + 0.5) * ss), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1]                      # sequential, in tap order (np.sum is pairwise)
    w = np.where((ww != 0.0)[:, None], w / np.where(ww != 0.0, ww, 1.0)[:, None], w)
    k = np.where(w < 0, np.trunc(w * (1 << PRECISION_BITS) - 0.5), np.trunc(w * (1 << PRECISION_BITS) + 0.5))
    k = np.where(live, k, 0.0).astype(np.int32)
    assert xmax.min() >= 1 and int((xmin + xmax).max()) <= n_in, (n_in, n_out, filt)
    return np.stack([xmin, xmax], 1).astype(np.int32), k


def _identity(o0, o1):
    idx = np.arange(o0, o1, dtype=np.int32)
    return np.stack([idx, np.ones_like(idx)], 1), np.full((o1 - o0, 1), 1 << PRECISION_BITS, np.int32)


class Pass:
    """One pass of a plan.  axis 0 filters along the rows (vertical), axis 1 along the columns (horizontal).  src_shape / dst_shape
    are (rows, columns) of the full images; the pass computes outputs [out0, out0 + nout) of its axis over [oth0, oth0 + noth) of the
    other one.  bounds[i] = (first source sample, taps) and coefs[i, :taps] belong to output out0 + i; source samples are absolute
    (a crop in front of the resize is already added)."""
    __slots__ = ("axis", "src_shape", "dst_shape", "out0", "nout", "oth0", "noth", "bounds", "coefs", "planar", "_filt", "_shift", "_n_in")

    def __init__(self, axis, src_shape, dst_shape, filt, shift=0, n_in=None):
        self.axis, self.src_shape, self.dst_shape = axis, tuple(src_shape), tuple(dst_shape)
        self._filt, self._shift, self._n_in = filt, shift, src_shape[axis] if n_in is None else n_in
        self.planar = False

    def finish(self, out0, nout, oth0, noth):
        """Fix the window and build the tables for it; returns the window of the source axis the pass reads."""
        self.out0, self.nout, self.oth0, self.noth = out0, nout, oth0, noth
        if self._filt is None:
            self.bounds, self.coefs = _identity(out0, out0 + nout)
        else:
            self.bounds, self.coefs = coefficients(self._n_in, self.dst_shape[self.axis], self._filt, out0, out0 + nout)
            self.bounds[:, 0] += self._shift
        lo, hi = int(self.bounds[:, 0].min()), int((self.bounds[:, 0] + self.bounds[:, 1]).max())
        assert lo >= 0 and hi <= self.src_shape[self.axis], (lo, hi, self.src_shape, self.axis)
        assert out0 >= 0 and out0 + nout <= self.dst_shape[self.axis] and oth0 >= 0 and oth0 + noth <= self.src_shape[1 - self.axis]
        return lo, hi - lo


def _resize_passes(passes, h, w, nh, nw, filt, crop=None):
    """The passes of Image.resize((nw, nh), filt) on an h x w image, `crop` = (y0, x0, ch, cw) taken first."""
    y0, x0, ch, cw = crop or (0, 0, h, w)
    if nw != cw:
        passes.append(Pass(1, (h, w), (h, nw), filt, shift=x0, n_in=cw))
        w, x0 = nw, 0
    if nh != ch:
        passes.append(Pass(0, (h, w), (nh, w), filt, shift=y0, n_in=ch))
        h, y0 = nh, 0
    return h, w, y0, x0


def plan(h, w, transform, R):
    """The passes that turn an h x w RGB image into the R x R crop of `transform`, first to last."""
    if transform not in TRANSFORMS:
        raise ValueError(f"transform {transform!r}: one of {TRANSFORMS}")
    if h < 1 or w < 1 or R < 4 or R % 4:
        raise ValueError(f"resample plan: {w}x{h} -> {R}: sizes must be positive and the resolution a multiple of 4")
    passes = []
    if transform == "center-crop-dhariwal":
        while min(w, h) >= 2 * R:
            h, w, _, _ = _resize_passes(passes, h, w, h // 2, w // 2, "box")
        sc = R / min(w, h)
        h, w, _, _ = _resize_passes(passes, h, w, round(h * sc), round(w * sc), "bicubic")
        y0, x0 = (h - R) // 2, (w - R) // 2
    else:
        c = min(h, w)
        h, w, y0, x0 = _resize_passes(passes, h, w, R, R, "lanczos", crop=((h - c) // 2, (w - c) // 2, c, c))   # c == R: no pass
    if y0 + R > h or x0 + R > w:
        raise ValueError(f"resample plan: the {R}x{R} crop does not fit the {w}x{h} result")
    if not passes or passes[-1].axis != 0:
        passes.append(Pass(0, (h, w), (h, w), None))          # one-tap identity: the crop / copy into the planar layout
    passes[-1].planar = True
    rows, cols = (y0, R), (x0, R)
    for p in reversed(passes):                                # trim every pass to what the later ones read
        if p.axis == 0:
            rows = p.finish(rows[0], rows[1], cols[0], cols[1])
        else:
            cols = p.finish(cols[0], cols[1], rows[0], rows[1])
    return passes


def execute_pass(cur, p):
    """One pass on cur u8 [rows, columns, 3] in numpy integers: the destination image, zero outside the pass's window."""
    assert cur.shape[:2] == p.src_shape
    dst = np.zeros(p.dst_shape + (3,), np.uint8)
    src = cur if p.axis == 0 else cur.transpose(1, 0, 2)
    out = dst if p.axis == 0 else dst.transpose(1, 0, 2)
    for i in range(p.nout):
        s0, n = int(p.bounds[i, 0]), int(p.bounds[i, 1])
        seg = src[s0:s0 + n, p.oth0:p.oth0 + p.noth].astype(np.int64)
        acc = (seg * p.coefs[i, :n].astype(np.int64)[:, None, None]).sum(0) + (1 << (PRECISION_BITS - 1))
        out[p.out0 + i, p.oth0:p.oth0 + p.noth] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return dst


def execute_plan(img, passes):
    """Run `passes` on img u8 [h, w, 3] in numpy integers; returns u8 [R, R, 3].  Outside a pass's window the intermediates hold
    zeros, which no later pass reads."""
    cur = np.ascontiguousarray(img)
    assert cur.dtype == np.uint8 and cur.ndim == 3 and cur.shape[2] == 3
    for p in passes:
        cur = execute_pass(cur, p)
    last = passes[-1]
    return np.ascontiguousarray(cur[last.out0:last.out0 + last.nout, last.oth0:last.oth0 + last.noth])


def pil_transform(img, transform, R):
    """The reference's make_transform through Pillow: u8 [h, w, 3] -> u8 [R, R, 3] (`--resize pil`, and the oracle in tests)."""
    import PIL.Image
    if transform == "center-crop-dhariwal":
        pil = PIL.Image.fromarray(img)
        while min(*pil.size) >= 2 * R:
            pil = pil.resize(tuple(x // 2 for x in pil.size), resample=PIL.Image.Resampling.BOX)
        sc = R / min(*pil.size)
        pil = pil.resize(tuple(round(x * sc) for x in pil.size), resample=PIL.Image.Resampling.BICUBIC)
        arr = np.array(pil)
        y0, x0 = (arr.shape[0] - R) // 2, (arr.shape[1] - R) // 2
        return np.ascontiguousarray(arr[y0:y0 + R, x0:x0 + R])
    if transform == "center-crop":
        c = min(img.shape[:2])
        img = img[(img.shape[0] - c) // 2:(img.shape[0] + c) // 2, (img.shape[1] - c) // 2:(img.shape[1] + c) // 2]
        return np.array(PIL.Image.fromarray(img, "RGB").resize((R, R), PIL.Image.Resampling.LANCZOS))
    raise ValueError(f"transform {transform!r}: one of {TRANSFORMS}")


# ---------------- the device side: tables of a ragged batch ----------------
def _up(n, a=ALIGN):
    return (n + a - 1) // a * a


def pitch_of(width):
    """Row pitch in bytes of an interleaved RGB image of `width` pixels in an arena."""
    return _up(3 * width)


def item_units(kind, out0, nout, oth0, noth):
    """Lanes' work items of one pass (csrc/resample.hip): a horizontal pass gives a lane 4 pixels at a multiple of 4, a vertical
    one a dword of the row's bytes, the planar one 4 pixels of the crop."""
    if kind == KIND_H:
        return noth * (((out0 + nout + 3) >> 2) - (out0 >> 2))
    if kind == KIND_V:
        return nout * (((3 * (oth0 + noth) + 3) >> 2) - ((3 * oth0) >> 2))
    return nout * (noth // 4)


TILE = 256   # work items per workgroup


class BatchPlan:
    """Everything `ops.resample_u8` needs for a ragged batch, in host arrays: per level the item table, the prefix of tile counts
    and the written regions; the concatenated coefficient and bounds tables; the layout of the three arenas."""

    def __init__(self, plans, R):
        self.n, self.R = len(plans), R
        self.src_off, off = [], 0
        for ps in plans:
            self.src_off.append(off)
            off += _up(ps[0].src_shape[0] * pitch_of(ps[0].src_shape[1]))
        self.src_bytes = off
        self.levels = []          # per level: (items int32 [n, ITEM_INTS], prefix of tile counts int32 [n + 1])
        coefs, bounds, ncoef, nbound = [], [], 0, 0
        self.scratch_bytes = [0, 0]
        prev_off = list(self.src_off)
        for lev in range(max(len(ps) for ps in plans)):
            rows, tiles, cur_off, fill = [], [], list(prev_off), 0
            for b, ps in enumerate(plans):
                if lev >= len(ps):
                    continue
                p = ps[lev]
                kind = KIND_H if p.axis == 1 else (KIND_V_PLANAR if p.planar else KIND_V)
                if kind == KIND_V_PLANAR:
                    assert lev == len(ps) - 1 and p.nout == R and p.noth == R
                    dst_off, dst_pitch, plane = b * 3 * R * R, R, R * R
                else:
                    dst_off, dst_pitch, plane = fill, pitch_of(p.dst_shape[1]), 0
                    fill += _up(p.dst_shape[0] * dst_pitch)
                    cur_off[b] = dst_off
                it = np.zeros(ITEM_INTS, np.int32)
                it[0:4] = np.array([prev_off[b], dst_off], np.int64).view(np.int32)
                it[4:] = [pitch_of(p.src_shape[1]), dst_pitch, p.src_shape[p.axis], p.out0, p.nout, p.oth0, p.noth, ncoef, nbound,
                          p.coefs.shape[1], kind, plane]
                rows.append(it)
                tiles.append(-(-item_units(kind, p.out0, p.nout, p.oth0, p.noth) // TILE))
                coefs.append(p.coefs.ravel())
                bounds.append(p.bounds.ravel())
                ncoef += p.coefs.size
                nbound += p.bounds.shape[0]
            self.scratch_bytes[lev % 2] = max(self.scratch_bytes[lev % 2], fill)
            self.levels.append((np.stack(rows), np.concatenate([[0], np.cumsum(tiles)]).astype(np.int32)))
            prev_off = cur_off
        self.coefs = np.concatenate(coefs).astype(np.int32)
        self.bounds = np.concatenate(bounds).astype(np.int32)
        self.out_bytes = self.n * 3 * R * R


def written_mask(level_items, nbytes, planar):
    """bool [nbytes]: the bytes of a level's destination arena (planar=False) or of the output (planar=True) that the level's
    launch writes: for each item the window of its pass, nothing else (no pitch padding, nothing outside the window)."""
    m = np.zeros(nbytes, bool)
    for it in level_items:
        dst_off = int(it[2:4].view(np.int64)[0])
        dst_pitch, out0, nout, oth0, noth, kind, plane = (int(it[5]), int(it[7]), int(it[8]), int(it[9]), int(it[10]), int(it[14]),
                                                          int(it[15]))
        if (kind == KIND_V_PLANAR) != planar:
            continue
        if kind == KIND_V_PLANAR:
            m[dst_off:dst_off + 3 * plane] = True
        elif kind == KIND_V:
            for y in range(out0, out0 + nout):
                m[dst_off + y * dst_pitch + 3 * oth0:dst_off + y * dst_pitch + 3 * (oth0 + noth)] = True
        else:
            for y in range(oth0, oth0 + noth):
                m[dst_off + y * dst_pitch + 3 * out0:dst_off + y * dst_pitch + 3 * (out0 + nout)] = True
    return m


class _Arenas:
    """Grow-only device and pinned buffers of center_crop_batch, per device."""

    def __init__(self):
        self.bufs = {}
        self.staged = None   # event behind the last copy out of the pinned staging buffer

    def get(self, name, nbytes, device, pinned=False):
        import torch
        t = self.bufs.get((name, str(device)))
        if t is None or t.numel() < nbytes:
            n = max(_up(nbytes, 1 << 20), 1 << 20)
            t = torch.empty(n, dtype=torch.uint8, pin_memory=True) if pinned else torch.empty(n, dtype=torch.uint8, device=device)
            self.bufs[(name, str(device))] = t
        return t


_ARENAS = _Arenas()


def stage_batch(images, bp, device):
    """Pack the pixels and every table of `bp` into the pinned staging buffer ([pixels | coefs | bounds | per level: items,
    prefix], each part 16-byte aligned) and copy it to the device in one piece; returns the device address of each part."""
    import torch
    parts, off = [], _up(bp.src_bytes)
    for arr in [bp.coefs, bp.bounds] + [a for lev in bp.levels for a in lev]:
        parts.append((off, arr))
        off += _up(arr.nbytes)
    if _ARENAS.staged is not None:
        _ARENAS.staged.synchronize()   # the previous batch's copy still reads the staging buffer
    stage = _ARENAS.get("stage", off, "cpu", pinned=True)
    host = stage.numpy()
    for im, o in zip(images, bp.src_off):
        h, w = im.shape[:2]
        host[o:o + h * pitch_of(w)].reshape(h, pitch_of(w))[:, :3 * w] = im.reshape(h, 3 * w)
    for o, arr in parts:
        host[o:o + arr.nbytes] = np.ascontiguousarray(arr).view(np.uint8).ravel()
    dev_in = _ARENAS.get("in", off, device)
    dev_in[:off].copy_(stage[:off], non_blocking=True)
    _ARENAS.staged = torch.cuda.Event()
    _ARENAS.staged.record()
    base = dev_in.data_ptr()
    return {"src": base, "coefs": base + parts[0][0], "bounds": base + parts[1][0],
            "levels": [(base + parts[2 + 2 * i][0], base + parts[3 + 2 * i][0]) for i in range(len(bp.levels))]}


def run_levels(bp, tables, scratch, out):
    """The launches of a staged batch: level 0 reads the staged pixels, level l > 0 the arena level l - 1 wrote."""
    from . import ops
    for lev, ((items, prefix), (d_items, d_prefix)) in enumerate(zip(bp.levels, tables["levels"])):
        src = tables["src"] if lev == 0 else scratch[(lev - 1) % 2].data_ptr()
        ops.resample_u8(src, scratch[lev % 2], out, d_items, d_prefix, items.shape[0], int(prefix[-1]), tables["coefs"],
                        tables["bounds"])


def center_crop_batch(images, transform, R, device="cuda", plans=None, out=None, scratch=None):
    """images: list of u8 [h, w, 3] arrays of any sizes -> u8 [B, 3, R, R] on `device`, the bytes Pillow gives (pil_transform).
    One pinned staging buffer and one host-to-device copy carry the pixels and every table; then one launch per pass level on
    two ping-pong scratch arenas, no synchronisation in between.  `plans` may carry plan() results computed elsewhere (the
    DataLoader workers); `out` (u8, >= B*3*R*R bytes) and `scratch` (two u8 tensors, large enough) replace the cached arenas."""
    import torch
    if not images:
        raise ValueError("center_crop_batch: no images")
    for im in images:
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            raise ValueError(f"center_crop_batch: images must be uint8 [h, w, 3], got {im.dtype} {im.shape}")
    if plans is None:
        plans = [plan(im.shape[0], im.shape[1], transform, R) for im in images]
    for im, ps in zip(images, plans):
        if ps[0].src_shape != im.shape[:2] or (ps[-1].nout, ps[-1].noth) != (R, R):
            raise ValueError(f"center_crop_batch: a plan for {ps[0].src_shape} -> {ps[-1].nout} with an image of {im.shape[:2]} -> {R}")
    bp = BatchPlan(plans, R)
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"center_crop_batch: device {device}: the resampler runs on the GPU (Pillow's path: pil_transform)")
    if scratch is None:
        scratch = [_ARENAS.get(f"scratch{i}", max(bp.scratch_bytes[i], ALIGN), device) for i in range(2)]
    if scratch[0].numel() < bp.scratch_bytes[0] or scratch[1].numel() < bp.scratch_bytes[1]:
        raise ValueError(f"center_crop_batch: scratch arenas of {bp.scratch_bytes} bytes needed")
    if out is None:
        out = torch.empty(bp.out_bytes, dtype=torch.uint8, device=device)
    if out.numel() < bp.out_bytes:
        raise ValueError(f"center_crop_batch: output of {bp.out_bytes} bytes needed")
    with torch.cuda.device(device):
        run_levels(bp, stage_batch(images, bp, device), scratch, out)
    return out[:bp.out_bytes].view(bp.n, 3, R, R)
