"""The images the resampler tests share: (R, width, height) of the cases, deterministic pixels (every second image thresholded to
0 / 255 so that both ends of the clip fire), and Pillow's result, computed once per (case, transform)."""
import functools

import numpy as np

# identity, upscaling, odd // 2 halvings with three-tap BOX rows, two halvings, a crop window far inside a strip
CASES = [(16, w, h) for w, h in [(37, 53), (53, 37), (16, 16), (15, 40), (9, 11), (131, 67), (64, 65), (33, 31), (129, 300), (17, 16),
                                 (31, 257)]] + [(32, 500, 375), (32, 63, 64), (8, 100, 7), (64, 333, 250)]
# the R = 16 cases plus one image larger than a workgroup tile (256 work items) in both directions: one mixed GPU batch
BATCH16 = [(w, h) for R, w, h in CASES if R == 16] + [(520, 260)]
TRANSFORMS = ("center-crop-dhariwal", "center-crop")


@functools.lru_cache(maxsize=None)
def image(w, h):
    rng = np.random.default_rng(1000 * w + h)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if (w + h) % 2:
        img = np.where(img > 127, 255, 0).astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def pillow(w, h, transform, R):
    from reed_amd import resample
    out = resample.pil_transform(np.array(image(w, h)), transform, R)
    out.setflags(write=False)
    return out
