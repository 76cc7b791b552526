"""Golden vectors for the edges of the score-image front end: outputs of Pillow itself (`Image.resize` of mode-"L" images, the
library the reference calls in src/data/preprocessing.py:44-52) at the window extremes, the clipping cases and the pass-order
case of tests/image_refs.py.  Run in the build container:  python tests/golden/gen_image_golden_edges.py
-> tests/golden/f11b_image.npz.  Pillow version recorded in the file.  No case has more than 2048 input pixels.

Per case NAME: NAME_pixels uint8 [h, w], NAME_size = (out_h, out_w), NAME_out uint8 [out_h, out_w] = resize((out_w, out_h)).
Cases whose out_w equals int(out_h * w / h) are what preprocess_image(pixels, out_h) computes: names starting with "sq_"."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import image_refs as R  # noqa: E402


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    cases = []                                                       # (name, pixels [h, w], out_h, out_w)
    rng = np.random.default_rng(20261021)
    for i, o in R.SIZE_PAIRS:
        for kind, row in (("noise", R.binary_noise(i)), ("random", rng.integers(0, 256, i, dtype=np.uint8))):
            cases.append((f"row_{kind}_{i}_{o}", row.reshape(1, i), 1, o))
            cases.append((f"col_{kind}_{i}_{o}", row.reshape(i, 1), o, 1))
    # 2-D, both passes, the width preprocess_image derives: w -> int(out_h * w / h)
    for h, w, oh in [(14, 14, 13), (5, 5, 64), (2, 10, 1), (1, 1, 7), (1, 3, 7), (37, 37, 96), (64, 32, 23), (317, 6, 137), (13, 13, 23), (2048, 1, 4096)]:
        cases.append((f"sq_noise_{h}x{w}_{oh}", R.binary_noise(h * w).reshape(h, w), oh, int(oh * w / h)))
    h, w, oh, ow = R.ORDER_SHAPE
    assert ow == int(oh * w / h)
    cases.append((f"sq_order_{h}x{w}_{oh}", R.order_pixels()[..., 0], oh, ow))
    for name, px, oh, ow in cases:
        assert px.size <= 2048 and ow >= 1 and oh >= 1, name
        got = np.asarray(Image.fromarray(np.ascontiguousarray(px)).resize((ow, oh))).copy()
        assert got.shape == (oh, ow) and got.dtype == np.uint8, name
        out[f"{name}_pixels"] = np.ascontiguousarray(px)
        out[f"{name}_size"] = np.array([oh, ow])
        out[f"{name}_out"] = got
    path = os.path.join(HERE, "f11b_image.npz")
    np.savez_compressed(path, **out)
    print("wrote f11b_image.npz:", len(cases), "cases,", os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
