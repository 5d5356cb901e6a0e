"""tests/augment_model.py against PIL over all 2^24 colours, both directions of the HSV round trip that the hue op of the
colour jitter takes: ``convert("HSV")`` of every RGB colour and ``convert("RGB")`` of every HSV triple.  CPU only, a few
seconds.  Prints one JSON line with the two mismatch counts (DESIGN.md records them: 0 and 0) and exits non-zero otherwise.

    python scripts/augment_model_sweep.py
"""
import json
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import augment_model as am  # noqa: E402


def main():
    import PIL

    a = np.arange(256, dtype=np.uint8)
    bad_fwd = bad_back = 0
    for first in range(256):  # one 256 x 256 slab per value of the first channel
        slab = np.empty((256, 256, 3), np.uint8)
        slab[..., 0], slab[..., 1], slab[..., 2] = first, a[:, None], a[None, :]
        bad_fwd += int((am.rgb_to_hsv(slab) != np.asarray(Image.fromarray(slab).convert("HSV"))).any(-1).sum())
        bad_back += int((am.hsv_to_rgb(slab) != np.asarray(Image.fromarray(slab, "HSV").convert("RGB"))).any(-1).sum())
    print(json.dumps(dict(pillow=PIL.__version__, colours=1 << 24, rgb_to_hsv_mismatches=bad_fwd, hsv_to_rgb_mismatches=bad_back)))
    return 0 if bad_fwd == bad_back == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
