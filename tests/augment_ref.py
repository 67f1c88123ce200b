"""CPU restatement of the training-batch builder (ppyolo_hip/augment.py + csrc/augment.hip) -- TEST INFRASTRUCTURE ONLY.

canvas(recipe): the pre-resize image of a planned sample, computed the way the reference's classes compute it
(tools/transform.py MixupImage / ColorDistort / RandomExpand / RandomCrop / RandomFlipImage on whole numpy arrays, numpy's
own dtype rules), from the uint8 BGR sources.  tests/test_augment_plan.py pins it to the reference (g19_augment).

resize(canvas, recipe): cv2.resize as OpenCV 4.x's scalar templates compute it, applied with the planner's coefficient
tables (augment.resize_plan).  PINNED: the tables against the interpolations' definitions in float64, to the measured bound of
tests/test_augment_cases.py (profiles/augment_resize_definition.txt); the 8-bit tables as the rounded float tables; the restated
8-bit CUBIC against oracle/preprocess_oracle.py.  NOT PINNED: OpenCV's own rounding inside its scalar templates (work types,
accumulation order, the 8-bit and integer-scale AREA roundings) -- cv2 is not installed in this image.

normalize(img): NormalizeImage + Permute of the reference (float32 / 255, float64 mean / std, rounded to float32)."""
import numpy as np

from ppyolo_hip import augment as A


def canvas(r, to_rgb=True):
    im = r['image'][:, :, ::-1] if to_rgb else r['image']
    if r['mix_image'] is not None:
        im2 = r['mix_image'][:, :, ::-1] if to_rgb else r['mix_image']
        f = r['factor']
        h, w = max(im.shape[0], im2.shape[0]), max(im.shape[1], im2.shape[1])
        img = np.zeros((h, w, 3), 'float32')
        img[:im.shape[0], :im.shape[1], :] = im.astype('float32') * f
        img[:im2.shape[0], :im2.shape[1], :] += im2.astype('float32') * (1.0 - f)
        im = img.astype('uint8')
    img = np.ascontiguousarray(im)
    for code, delta, t in r['ops']:
        img = img.astype(np.float32)
        if code == A.OP_BRIGHTNESS:
            img += delta
        elif code == A.OP_CONTRAST:
            img *= delta
        elif code == A.OP_SATURATION:
            gray = img * np.array([[[0.299, 0.587, 0.114]]], dtype=np.float32)
            gray = gray.sum(axis=2, keepdims=True)
            gray *= (1.0 - delta)
            img *= delta
            img += gray
        else:
            img = np.dot(img, t)
    if r['expand'] is not None:
        h, w, y, x = r['expand']
        cv = np.ones((h, w, 3), dtype=np.uint8)
        cv *= r['fill']
        cv[y:y + img.shape[0], x:x + img.shape[1], :] = img.astype(np.uint8)
        img = cv
    cy, cx, ch, cw = r['crop']
    img = img[cy:cy + ch, cx:cx + cw, :]
    if r['flip']:
        img = img[:, ::-1, :]
    return np.ascontiguousarray(img)


def resize(img, r):
    """-> resized [S,S,3] in the canvas dtype (uint8 / float32 / float64)."""
    p = r['resize']
    h, w = img.shape[:2]
    xi = lambda k: np.clip(p['xfirst'] + k, 0, w - 1)
    yi = lambda k: np.clip(p['yfirst'] + k, 0, h - 1)
    if p['mode'] == A.MODE_NEAREST:
        return img[p['yfirst']][:, p['xfirst']]
    if p['mode'] == A.MODE_AREA_FAST:
        ix, iy = p['ix'], p['iy']
        if img.dtype == np.uint8:
            s = np.zeros((len(p['yfirst']), len(p['xfirst']), 3), np.int64)
            for yy in range(iy):
                for xx in range(ix):
                    s += img[yi(yy)][:, xi(xx)]
            if ix == 2 and iy == 2:
                return np.clip((s + 2) >> 2, 0, 255).astype(np.uint8)
            return np.clip(np.rint(s.astype(np.float32) * np.float32(1.0 / (ix * iy))), 0, 255).astype(np.uint8)
        s = np.zeros((len(p['yfirst']), len(p['xfirst']), 3), img.dtype)
        for yy in range(iy):
            for xx in range(ix):
                s = s + img[yi(yy)][:, xi(xx)]
        return (s * img.dtype.type(np.float32(1.0) / np.float32(ix * iy))).astype(img.dtype)
    kx, ky = p['xw'].shape[1], p['yw'].shape[1]
    if img.dtype == np.uint8 and p['fixpt']:
        src = img.astype(np.int64)
        hor = sum(src[:, xi(j)] * p['xw'][:, j].astype(np.int64)[None, :, None] for j in range(kx))
        acc = sum(hor[yi(k)] * p['yw'][:, k].astype(np.int64)[:, None, None] for k in range(ky))
        return np.clip((acc + (1 << 21)) >> 22, 0, 255).astype(np.uint8)
    wt = np.float64 if img.dtype == np.float64 else np.float32
    src = img.astype(wt)
    hor = src[:, xi(0)] * p['xw'][:, 0].astype(wt)[None, :, None]
    for j in range(1, kx):
        hor = hor + src[:, xi(j)] * p['xw'][:, j].astype(wt)[None, :, None]
    acc = hor[yi(0)] * p['yw'][:, 0].astype(wt)[:, None, None]
    for k in range(1, ky):
        acc = acc + hor[yi(k)] * p['yw'][:, k].astype(wt)[:, None, None]
    if img.dtype == np.uint8:
        return np.clip(np.rint(acc), 0, 255).astype(np.uint8)
    return acc


def normalize(img, mean, std, is_scale=True):
    im = img.astype(np.float32, copy=False)
    mean = np.array(mean)[np.newaxis, np.newaxis, :]
    std = np.array(std)[np.newaxis, np.newaxis, :]
    if is_scale:
        im = im / 255.0
    im -= mean
    im /= std
    return np.ascontiguousarray(np.swapaxes(np.swapaxes(im, 1, 2), 1, 0))


def images(recipes, mean, std, to_rgb=True):
    return np.stack([normalize(resize(canvas(r, to_rgb), r), mean, std) for r in recipes])
