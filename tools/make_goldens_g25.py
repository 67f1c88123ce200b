"""tests/golden/g25_pil_resize.npz: seeded uint8 inputs and what Pillow's Image.resize returns for them, for the small cases
of tests/pil_resize_ref.py (every filter, random and binary 0 / 255 content).  With it the pin of the device resize
(csrc/pil_resize.hip) and of the numpy restatement does not move with the installed Pillow; the generating version is recorded.

    python tools/make_goldens_g25.py            # needs Pillow; writes the file and prints its size
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import pil_resize_ref as ref  # noqa: E402


def main():
    import PIL
    from PIL import Image
    out = {'pillow_version': np.array(PIL.__version__)}
    for (h, w), (ow, oh) in ref.SMALL_CASES:
        for kind in ('random', 'binary'):
            key = '%dx%d_%dx%d_%s' % (h, w, ow, oh, kind)
            img = ref.content(h, w, kind, ref.case_seed(h, w, ow, oh))
            out['in_' + key] = img
            for f in ref.FILTERS:
                out['out_%s_f%d' % (key, f)] = np.asarray(Image.fromarray(img).resize((ow, oh), f))
    path = os.path.join(ROOT, 'tests', 'golden', 'g25_pil_resize.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes, Pillow %s' % (path, len(out), os.path.getsize(path), PIL.__version__))


if __name__ == '__main__':
    main()
