"""`multiclass_nms`: PaddleDetection's greedy per-class hard NMS for one image, the twin of model/matrix_nms.py, executed by
the HIP kernels (ppy_nms_candidates_f32 + ppy_multiclass_nms_f32).  boxes [M,4] xyxy, scores [M,C] on a ROCm device ->
[K,6] rows (label, score, x0,y0,x1,y1) in (class ascending, score descending, box index ascending) order, or [[-1]*6].

Per class != background_label: the boxes with score > score_threshold by (score descending, box index ascending), the
first nms_top_k of them, then a box is selected iff its IoU with every box already selected in that class is <=
nms_threshold (`normalized=False` adds 1 to every width and height: pixel coordinates).  Across classes the keep_top_k
highest scores stay (ties to the lower class).  Scores are returned unchanged.

Supported: 1 <= nms_top_k <= 1024, 1 <= keep_top_k <= 1024, nms_eta == 1.0 (no adaptive threshold).  Paddle's -1 ("no
limit") for nms_top_k / keep_top_k is therefore NOT accepted: PPYoloHipError names the parameter, nothing is clamped."""
import torch

from ppyolo_hip import ops


def multiclass_nms(bboxes, scores, score_threshold, nms_top_k, keep_top_k, nms_threshold=0.3, normalized=True, nms_eta=1.0,
                   background_label=-1, return_index=False):
    M, C = scores.shape
    dev = bboxes.device
    b = bboxes.detach().float().contiguous().view(1, M, 4)
    s = scores.detach().float().contiguous().view(1, M, C)
    kk = max(int(keep_top_k), 1)          # (an unsupported keep_top_k is refused by the call below, not by an allocation)
    ck = torch.zeros((1, M * C), dtype=torch.int32, device=dev)
    ci = torch.zeros((1, M * C), dtype=torch.int32, device=dev)
    cc = torch.zeros((1,), dtype=torch.int32, device=dev)
    dets = torch.zeros((1, kk, 6), dtype=torch.float32, device=dev)
    cnt = torch.zeros((1,), dtype=torch.int32, device=dev)
    keep = torch.zeros((1, kk), dtype=torch.int32, device=dev)
    ops.nms_candidates(s, score_threshold, ck, ci, cc)
    ops.multiclass_nms(b, C, ck, ci, cc, nms_top_k, keep_top_k, nms_threshold, normalized, nms_eta, background_label, dets,
                       cnt, keep)
    k = int(cnt.item())
    pred = dets[0, :max(k, 1)].clone()
    return (pred, keep[0, :k].clone()) if return_index else pred
