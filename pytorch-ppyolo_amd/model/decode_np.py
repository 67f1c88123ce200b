"""Host harness boundary -- the part of the reference's `model/decode_np.py` that sits on the
model boundary: `Decode.predict` (:142-150), `detect_image` (:41-57), `detect_batch`
(:81-96), and `process_image` (:125-140) -- the cv2 resize / normalise / permute in front of the
model, here ONE HIP kernel on the device (ppyolo_hip/csrc/preprocess.hip; SURVEY.md section 8f
rank 1) -- and `draw` (:98-123) as one HIP launch (ppyolo_hip/draw.py): the reference's boxes, colours, label strings and
placement, with Pillow's bitmap font where the reference calls cv2.putText (cv2's glyphs are not pinned: DESIGN.md 10c)."""
import numpy as np
import torch


class Decode(object):
    def __init__(self, _yolo, all_classes, use_gpu, cfg, for_test=True):
        self.all_classes = all_classes
        self.num_classes = len(all_classes)
        self._yolo = _yolo
        self.use_gpu = use_gpu
        self.cfg = cfg
        # reference :32-37: eval target size unless for_test
        self.target_size = (cfg.test_cfg if for_test else cfg.eval_cfg)['target_size']
        self._pre = None
        self._jpeg = None
        self._drawer = None
        self._encoder = None

    def _preprocessor(self):
        if self._pre is None:
            from ppyolo_hip.preprocess import Preprocessor
            self._pre = Preprocessor(self.cfg, self.target_size)
        return self._pre

    def process_image(self, img, to_numpy=True):
        """uint8 BGR [h,w,3] -> (pimage [1,3,S,S] float32, im_size [[h, w]] int32), computed on the device.
        `to_numpy=True` returns numpy arrays like the reference; False keeps pimage on the device (what `predict`
        wants anyway) and saves the round trip."""
        pimage, _ = self._preprocessor()([img])
        im_size = np.array([[img.shape[0], img.shape[1]]]).astype(np.int32)
        return (pimage.cpu().numpy() if to_numpy else pimage), im_size

    def detect_raw(self, images):
        """Throughput form of demo.py's loop: raw uint8 BGR images of any sizes -> per image (boxes, scores, classes),
        pre-processing, forward and Matrix-NMS all on the device."""
        pimage, im_size = self._preprocessor()(images)
        preds = self._yolo(pimage, im_size)
        return [self._split(p.cpu().detach().numpy()) for p in preds]

    def detect_files(self, paths_or_bytes, decoder=None):
        """demo.py's loop from the files themselves: JPEG paths / byte strings -> decoded on the device
        (ppyolo_hip/jpeg.py, the pixels cv2.imread gives) -> detect_raw.  A file outside the decoder's subset raises
        PPYoloHipError naming the reason.  decoder: a JpegDecoder of the caller's (JpegDecoder(entropy='device'), say);
        default one of this object's own with the default settings."""
        if decoder is None:
            if self._jpeg is None:
                from ppyolo_hip.jpeg import JpegDecoder
                self._jpeg = JpegDecoder()
            decoder = self._jpeg
        return self.detect_raw(decoder.decode(list(paths_or_bytes)))

    def predict(self, image, im_size):
        """numpy [N,3,S,S] f32 + numpy [N,2] (h, w) -> list of numpy [K,6] f32."""
        if not isinstance(image, torch.Tensor):
            image = torch.as_tensor(np.asarray(image), dtype=torch.float32)
        im_size = torch.as_tensor(np.asarray(im_size), dtype=torch.float32)
        if not self.use_gpu:
            raise RuntimeError('the MI355X path has no CPU mode: construct Decode(use_gpu=True)')
        image, im_size = image.cuda(), im_size.cuda()
        preds = self._yolo(image, im_size)
        return [p.cpu().detach().numpy() for p in preds]

    @staticmethod
    def _split(pred):
        if pred[0][0] < 0.0:                      # the [[-1]*6] "no detection" row
            return np.array([]), np.array([]), np.array([])
        return pred[:, 2:], pred[:, 1], pred[:, 0].astype(np.int32)

    def drawer(self):
        if self._drawer is None:
            from ppyolo_hip.draw import BoxDrawer
            self._drawer = BoxDrawer(self.all_classes)
        return self._drawer

    def draw(self, image, boxes, scores, classes):
        """Reference :98-123, in place: every row given is drawn, in order.  image: a numpy uint8 [h,w,3] array (uploaded, drawn
        on the device, copied back into the same array) or a uint8 device tensor (drawn where it lies)."""
        if isinstance(image, torch.Tensor):
            return self._draw_tensor(image, boxes, scores, classes)
        return self.drawer().draw_host(image, boxes, scores, classes)

    def _draw_tensor(self, image, boxes, scores, classes):
        scores = np.asarray(scores, np.float32).reshape(-1)
        rows = np.concatenate([np.asarray(classes, np.float32).reshape(-1, 1), scores[:, None],
                               np.asarray(boxes, np.float32).reshape(-1, 4)], axis=1)
        for lo in range(0, len(rows), 1024):       # the launch takes 1024 rows; in order on one stream, as draw_host does
            dets = torch.from_numpy(np.ascontiguousarray(rows[lo:lo + 1024])[None]).to(image.device)
            count = torch.tensor([dets.shape[1]], dtype=torch.int32, device=image.device)
            self.drawer()([image], dets, count, 0.0)
        return image

    def _draw_filtered(self, image, boxes, scores, classes, draw_thresh):
        if len(scores) > 0:                       # reference :51-56
            pos = np.where(scores >= draw_thresh)
            self.draw(image, boxes[pos], scores[pos], classes[pos])

    def detect_image(self, image, pimage, im_size, draw_image, draw_thresh=0.0):
        pred = self.predict(pimage, im_size)
        boxes, scores, classes = self._split(pred[0])
        if draw_image:
            self._draw_filtered(image, boxes, scores, classes, draw_thresh)
        return image, boxes, scores, classes

    def detect_batch(self, batch_img, batch_pimage, batch_im_size, draw_image, draw_thresh=0.0):
        pred = self.predict(batch_pimage, batch_im_size)
        res = [self._split(p) for p in pred]
        if draw_image:
            for img, (boxes, scores, classes) in zip(batch_img, res):
                self._draw_filtered(img, boxes, scores, classes, draw_thresh)
        return (list(batch_img), [r[0] for r in res], [r[1] for r in res], [r[2] for r in res])

    def annotate_files(self, paths_or_bytes, draw_thresh=None, decoder=None, encoder=None):
        """demo.py's loop from file to annotated file: JPEG paths / byte strings -> (list of JPEG bytes, per image (boxes,
        scores, classes)).  decode -> preprocess -> forward_padded -> draw -> JpegEncoder.encode, all on the device: no pixel
        and no score visits the host before the encoder's read-back; the detections are read after it.  draw_thresh: default
        cfg.test_cfg['draw_thresh'].  decoder / encoder: the caller's JpegDecoder / JpegEncoder; default this object's own
        (the encoder with cv2.imwrite's defaults, quality 95 and 4:2:0)."""
        if draw_thresh is None:
            draw_thresh = self.cfg.test_cfg['draw_thresh']
        if decoder is None:
            if self._jpeg is None:
                from ppyolo_hip.jpeg import JpegDecoder
                self._jpeg = JpegDecoder()
            decoder = self._jpeg
        if encoder is None:
            if self._encoder is None:
                from ppyolo_hip.jpeg import JpegEncoder
                self._encoder = JpegEncoder()
            encoder = self._encoder
        images = decoder.decode(list(paths_or_bytes))
        pimage, im_size = self._preprocessor()(images)
        dets, count, _ = self._yolo.forward_padded(pimage, im_size)
        self.drawer()(images, dets, count, draw_thresh)
        files = encoder.encode(images)
        dets, count = dets.cpu().numpy(), count.cpu().tolist()
        empty = (np.array([]), np.array([]), np.array([]))
        return files, [self._split(d[:c]) if c > 0 else empty for d, c in zip(dets, count)]

    def crop_files(self, paths_or_bytes, size, filter=3, pad=0.0, draw_thresh=None, decoder=None, encoder=None):
        """From file to one JPEG file per detection: JPEG paths / byte strings -> (per image the list of JPEG bytes of its
        detections with score >= draw_thresh, in row order, each resized to size = (ow, oh) with Pillow's `filter` (default
        BICUBIC) and `pad`; per image (boxes, scores, classes) as annotate_files returns them).  decode -> preprocess ->
        forward_padded -> DetectionCropper -> JpegEncoder.encode, on the device: the crops are cut from the undrawn source
        pixels, the boxes never visit the host, and the first read-back is the crop list's (ppyolo_hip/crops.py)."""
        from ppyolo_hip.crops import DetectionCropper
        if draw_thresh is None:
            draw_thresh = self.cfg.test_cfg['draw_thresh']
        if decoder is None:
            if self._jpeg is None:
                from ppyolo_hip.jpeg import JpegDecoder
                self._jpeg = JpegDecoder()
            decoder = self._jpeg
        if encoder is None:
            if self._encoder is None:
                from ppyolo_hip.jpeg import JpegEncoder
                self._encoder = JpegEncoder()
            encoder = self._encoder
        key = (tuple(size), filter, pad)
        if getattr(self, '_cropper_key', None) != key:
            self._cropper, self._cropper_key = DetectionCropper(size, filter=filter, pad=pad), key
        images = decoder.decode(list(paths_or_bytes))
        pimage, im_size = self._preprocessor()(images)
        dets, count, _ = self._yolo.forward_padded(pimage, im_size)
        crops, src, total = self._cropper(images, dets, count, draw_thresh)
        per_image = self._cropper.split(crops, src, total)
        flat = [c for _, group in per_image for c in group.unbind(0)]
        encoded = encoder.encode(flat) if flat else []
        files, at = [], 0
        for rows, _ in per_image:
            files.append(encoded[at:at + len(rows)])
            at += len(rows)
        dets, count = dets.cpu().numpy(), count.cpu().tolist()
        empty = (np.array([]), np.array([]), np.array([]))
        return files, [self._split(d[:c]) if c > 0 else empty for d, c in zip(dets, count)]

    def tiled_detector(self, **kw):
        """The TiledDetector (ppyolo_hip/tiles.py) of these settings; it is kept, keyed by its settings, as crop_files keeps its
        cropper."""
        from ppyolo_hip.tiles import TiledDetector
        key = tuple(sorted(kw.items()))
        if getattr(self, '_tiled_key', None) != key:
            self._tiled, self._tiled_key = TiledDetector(self._yolo, self.cfg, self.target_size, **kw), key
        return self._tiled

    def detect_tiled(self, images, **kw):
        """detect_raw for images larger than the network input: every image is cut into overlapping tiles (plus the whole
        image), the views run through the network at native resolution and their rows are merged on the device.  images: uint8
        BGR [h,w,3] device tensors (read in place) or numpy arrays; kw: TiledDetector's settings (tile, overlap, full_view, metric,
        thresh, score_thresh, keep_top_k, class_agnostic, batch).  Returns per image (boxes, scores, classes) in image pixels."""
        dets, count, _ = self.tiled_detector(**kw)(images)
        dets, count = dets.cpu().numpy(), count.cpu().tolist()
        empty = (np.array([]), np.array([]), np.array([]))
        return [self._split(d[:c]) if c > 0 else empty for d, c in zip(dets, count)]

    def detect_tiled_files(self, paths_or_bytes, decoder=None, **kw):
        """detect_tiled from the files themselves, decoded on the device as detect_files does."""
        if decoder is None:
            if self._jpeg is None:
                from ppyolo_hip.jpeg import JpegDecoder
                self._jpeg = JpegDecoder()
            decoder = self._jpeg
        return self.detect_tiled(decoder.decode(list(paths_or_bytes)), **kw)

    def tta_detector(self, **kw):
        """The TtaDetector (ppyolo_hip/tta.py) of these settings (scales: default this object's target size); it is kept, keyed
        by its settings, as tiled_detector keeps its own."""
        from ppyolo_hip.tta import TtaDetector
        kw.setdefault('scales', (self.target_size,))
        key = repr(sorted(kw.items()))
        if getattr(self, '_tta_key', None) != key:
            self._tta, self._tta_key = TtaDetector(self._yolo, self.cfg, **kw), key
        return self._tta

    def detect_tta(self, images, **kw):
        """detect_raw with test-time augmentation: every image runs through the network at every input side of `scales`, plain
        and mirrored, and the views' rows are fused on the device (weighted boxes fusion).  images: uint8 BGR [h,w,3] device
        tensors (read in place) or numpy arrays; kw: TtaDetector's settings (scales, hflip, weights, thresh, score_thresh,
        keep_top_k, batch).  Returns per image (boxes, scores, classes) in image pixels; a score is the cluster's confidence."""
        dets, count, _, _ = self.tta_detector(**kw)(images)
        dets, count = dets.cpu().numpy(), count.cpu().tolist()
        empty = (np.array([]), np.array([]), np.array([]))
        return [self._split(d[:c]) if c > 0 else empty for d, c in zip(dets, count)]

    def detect_tta_files(self, paths_or_bytes, decoder=None, **kw):
        """detect_tta from the files themselves, decoded on the device as detect_files does."""
        if decoder is None:
            if self._jpeg is None:
                from ppyolo_hip.jpeg import JpegDecoder
                self._jpeg = JpegDecoder()
            decoder = self._jpeg
        return self.detect_tta(decoder.decode(list(paths_or_bytes)), **kw)
