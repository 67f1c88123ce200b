"""The seeded inputs of the JPEG encoder tests: one place, so the restatement test, the golden maker and the GPU tests agree on
them.  numpy only."""
import numpy as np

QUALITIES = (1, 24, 25, 49, 50, 75, 95, 100)
SAMPLINGS = ('4:4:4', '4:2:2', '4:2:0', 'grey')
RESTARTS = (0, 1, 3)
SIZES = ((1, 1), (7, 9), (8, 8), (9, 8), (8, 9), (16, 16), (17, 1), (1, 17), (33, 35), (65, 33))          # (width, height)
CONTENTS = ('smooth', 'noise', 'flat', 'checker')


def image(content, w, h, grey, seed=0):
    """uint8 [h,w,3] BGR, or [h,w] with grey=True."""
    rng = np.random.default_rng([seed, w, h, CONTENTS.index(content), int(grey)])
    c = 1 if grey else 3
    if content == 'smooth':
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([127 + 100 * np.sin(x / (5.0 + k) + k) * np.cos(y / (7.0 - k)) + rng.normal(0, 2, (h, w)) for k in range(c)], -1)
    elif content == 'noise':
        a = rng.integers(0, 256, (h, w, c))
    elif content == 'flat':
        a = np.broadcast_to(rng.integers(0, 256, c), (h, w, c))
    else:                                   # every 8x8 block of every channel 0 or 255, opposite to its neighbours
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([255 * ((y // 8 + x // 8 + (k == 1)) & 1) for k in range(c)], -1)
    a = np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(a[..., 0] if grey else a)


def grid():
    """(name, content, w, h, sampling, quality, restart): the whole grid of the issue; the checkerboard at quality 100 only."""
    for content in CONTENTS:
        for w, h in SIZES:
            for s in SAMPLINGS:
                for q in ((100,) if content == 'checker' else QUALITIES):
                    for r in RESTARTS:
                        yield '%s_%dx%d_%s_q%d_r%d' % (content, w, h, s.replace(':', ''), q, r), content, w, h, s, q, r


def golden_subset():
    """The cases stored in tests/golden/g21_jpeg_encode.npz: every size with every sampling once, the qualities, restart
    intervals and the first three contents taken in turn, and the checkerboard at the three largest sizes."""
    k = 0
    for w, h in SIZES:
        for s in SAMPLINGS:
            content, q, r = CONTENTS[k // 3 % 3], QUALITIES[k % len(QUALITIES)], RESTARTS[k % len(RESTARTS)]
            yield '%s_%dx%d_%s_q%d_r%d' % (content, w, h, s.replace(':', ''), q, r), content, w, h, s, q, r
            k += 1
    for w, h in SIZES[-3:]:
        for s in SAMPLINGS:
            r = RESTARTS[k % len(RESTARTS)]
            yield 'checker_%dx%d_%s_q100_r%d' % (w, h, s.replace(':', ''), r), 'checker', w, h, s, 100, r
            k += 1


# the COCO-sized decoder fixtures (tests/golden/g20_jpeg.npz): their decoded pixels, encoded with the defaults
COCO = (('coco_398725', '4:2:0', 95, 0), ('coco_54592', '4:2:0', 95, 0))


# ---- tests/golden/g21_jpeg_encode.npz (tools/make_jpeg_encode_goldens.py) as the tests read it --------------------------
_G = None


def golden():
    global _G
    if _G is None:
        import os
        _G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g21_jpeg_encode.npz'))
    return _G


def golden_cases():
    """[(name, subsampling, quality, restart interval)] of the cases stored with pixels and bytes."""
    return [(str(n), str(s), int(q), int(r)) for n, s, q, r in golden()['cases']]


def golden_pixels(name):
    return golden()['px_' + name]


def golden_bytes(name):
    return golden()['jpg_' + name].tobytes()


def matches_coco(name, data):
    """data == the file libjpeg-turbo wrote from the COCO-sized fixture's pixels (stored as length and SHA-256)."""
    import hashlib
    g = golden()
    return len(data) == int(g['len_' + name]) and hashlib.sha256(data).hexdigest() == str(g['sha_' + name])
