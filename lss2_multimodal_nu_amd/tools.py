"""Host-side mirror of the hot-path helpers of the reference's `src/tools.py`
(`gen_dx_bx` :172-178, `cumsum_trick` :181-189, `QuickCumsum` :192-218).

`gen_dx_bx` is init-time host arithmetic.  `cumsum_trick` / `QuickCumsum` keep
the reference's call signature for callers that still drive the splat through
them; the sums run in the HIP segmented-sum kernel (direct per-run sums, not a
cumsum followed by differences - ~1000x less rounding noise).
The fused `LSS.forward` path does not go through them at all.
"""
import os

import torch

from . import ops


def gen_dx_bx(xbound, ybound, zbound):
    """Voxel size `dx`, first voxel centre `bx` (fp32) and voxel counts `nx`
    (int64) of a grid given as three [lo, hi, step] triples."""
    bounds = (xbound, ybound, zbound)
    dx = torch.tensor([b[2] for b in bounds], dtype=torch.float32)
    bx = torch.tensor([b[0] + b[2] / 2.0 for b in bounds], dtype=torch.float32)
    # float division then truncation, as LongTensor(list of floats) does
    nx = torch.tensor([int((b[1] - b[0]) / b[2]) for b in bounds], dtype=torch.int64)
    return dx, bx, nx


def _runs(ranks):
    """Boundaries of the equal-rank runs of a sorted rank vector: `last` marks the
    final row of every run, `seg_start` (M+1 int32) the row offsets."""
    K = ranks.shape[0]
    last = torch.ones(K, device=ranks.device, dtype=torch.bool)
    if K > 1:
        last[:-1] = ranks[1:] != ranks[:-1]
    ends = torch.nonzero(last).flatten()
    seg_start = torch.cat([ends.new_zeros(1), ends + 1]).to(torch.int32)
    return last, seg_start


def _segmented(x, seg_start):
    if not x.is_cuda:
        raise RuntimeError("cumsum_trick / QuickCumsum run on the GPU (HIP segmented-sum kernel); "
                           "got a %s tensor" % x.device)
    return ops.segmented_sum(x.contiguous().float(), seg_start)


def cumsum_trick(x, geom_feats, ranks):
    """Per-voxel sums of rows pre-sorted by `ranks`; returns (sums, geom of each run)."""
    last, seg_start = _runs(ranks)
    return _segmented(x, seg_start), geom_feats[last]


class QuickCumsum(torch.autograd.Function):
    """Same contract as the reference's autograd.Function: forward = per-run sums,
    backward = every row receives its run's gradient."""

    @staticmethod
    def forward(ctx, x, geom_feats, ranks):
        last, seg_start = _runs(ranks)
        y = _segmented(x, seg_start)
        geom_kept = geom_feats[last]
        ctx.save_for_backward(last)
        ctx.mark_non_differentiable(geom_kept)
        return y, geom_kept

    @staticmethod
    def backward(ctx, gradx, gradgeom):
        last, = ctx.saved_tensors
        run_of_row = torch.cumsum(last, 0) - last.to(torch.int64)
        return gradx[run_of_row], None, None


class _WeightedCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight):
        x = logits.float().contiguous()
        t = target.contiguous()
        w = weight.float().contiguous()
        loss, sums = ops.weighted_ce_fwd(x, t, w)
        ctx.save_for_backward(x, t, w, sums)
        ctx.in_dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        x, t, w, sums = ctx.saved_tensors
        gx = ops.weighted_ce_bwd(x, t, w, sums, g)
        return gx.to(ctx.in_dtype), None, None


def weighted_cross_entropy(ypred, ytgt, weight):
    """nn.CrossEntropyLoss(weight=weight)(ypred, ytgt) for (B,C,H,W) logits / (B,H,W) int64 targets:
    one HIP pass forward, one backward on the GPU (csrc/loss.hip); torch's own op elsewhere."""
    if ypred.is_cuda and ypred.dim() >= 3 and ypred.shape[1] <= 16 and ytgt.dtype == torch.int64:
        return _WeightedCEFn.apply(ypred, ytgt, weight)
    return torch.nn.functional.cross_entropy(ypred, ytgt, weight=weight)


class _HeadCEFn(torch.autograd.Function):
    """loss = CrossEntropy(weight)(conv1x1(y; W, b), target) with the head and the loss in ONE HIP pass each way
    (csrc/loss.hip: lss_head_ce_fwd / _bwd).  y: logical (B, Cin, H, W) tensor whose memory is NHWC bf16 (what the
    conv + BatchNorm + ReLU training unit hands over); W (K, Cin, 1, 1), b (K)."""

    @staticmethod
    def forward(ctx, y, weight, bias, target, class_w):
        yn = y.permute(0, 2, 3, 1)
        if yn.dtype != torch.bfloat16:
            yn = yn.to(torch.bfloat16)
        yn = yn.contiguous()
        w2 = weight.detach().float().reshape(weight.shape[0], -1).contiguous()
        b1 = bias.detach().float().contiguous()
        cw = class_w.detach().float().contiguous()
        t = target.contiguous()
        loss, sums = ops.head_ce_fwd(yn, w2, b1, t, cw)
        ctx.save_for_backward(yn, w2, b1, t, cw, sums)
        ctx.meta = (y.dtype, weight.shape, weight.dtype, bias.dtype)
        return loss

    @staticmethod
    def backward(ctx, g):
        yn, w2, b1, t, cw, sums = ctx.saved_tensors
        ydt, wshape, wdt, bdt = ctx.meta
        dy, dw, db = ops.head_ce_bwd(yn, w2, b1, t, cw, sums, g)
        dy = dy.permute(0, 3, 1, 2)
        return (dy if dy.dtype == ydt else dy.to(ydt)), dw.view(wshape).to(wdt), db.to(bdt), None, None


class _Head1x1Fn(torch.autograd.Function):
    """`head(y)` for the 1x1 head `nn.Conv2d(128, K, 1)` (ref src/modules.py:115; with 64 channels the `seg_head[6]` of
    BEVEncoderTransformer, ref src/model_vovnet_transformer.py:143) on the HIP kernels, both ways: the
    logits of a training-mode `model(x)` whose loss the caller computes (ref train.py:52, 62).  y: logical
    (B, Cin, H, W) tensor whose memory is NHWC bf16; returns (B, K, H, W) fp32.  Replaces torch's convolution there
    because the library's backward is not safe inside a HIP graph: round 3's data-parallel graph step went wrong in
    exactly this op."""

    @staticmethod
    def forward(ctx, y, weight, bias):
        yn = y.permute(0, 2, 3, 1)
        if yn.dtype != torch.bfloat16:
            yn = yn.to(torch.bfloat16)
        yn = yn.contiguous()
        w2 = weight.detach().float().reshape(weight.shape[0], -1).contiguous()
        b1 = bias.detach().float().contiguous()
        out = ops.head1x1_fwd(yn, w2, b1)
        ctx.save_for_backward(yn, w2, b1)
        ctx.meta = (y.dtype, weight.shape, weight.dtype, bias.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        yn, w2, b1 = ctx.saved_tensors
        ydt, wshape, wdt, bdt = ctx.meta
        dy, dw, db = ops.head1x1_bwd(yn, w2, b1, g.float().contiguous())
        dy = dy.permute(0, 3, 1, 2)
        return (dy if dy.dtype == ydt else dy.to(ydt)), dw.view(wshape).to(wdt), db.to(bdt)


def head_1x1(y, head):
    """head(y) on the autograd path: the HIP head kernels when the shapes fit (64 or 128 input channels, 4 or 8 classes,
    a bf16 activation on the GPU), torch's convolution otherwise (fp32 parity mode, or LSS_TRAIN_NATIVE=0 - the
    library comparison leg of the tests; NOT safe inside a HIP graph)."""
    if (os.environ.get("LSS_TRAIN_NATIVE", "1") != "0" and y.is_cuda and y.dtype == torch.bfloat16 and y.dim() == 4 and y.shape[1] in (64, 128) and head.kernel_size == (1, 1)
            and head.stride == (1, 1) and head.bias is not None and head.out_channels in (4, 8)):
        return _Head1x1Fn.apply(y, head.weight, head.bias)
    return head(y)


def head_weighted_cross_entropy(y, head, ytgt, weight):
    """nn.CrossEntropyLoss(weight=weight)(head(y), ytgt) for a 1x1 `head` = nn.Conv2d(Cin, K, 1) applied to the
    (B, Cin, H, W) activation y: fused into one HIP kernel per direction on the GPU when the shapes
    fit (64 or 128 input channels, 4 or 8 classes) AND y is already bf16 (autocast / bf16 precision: the kernel reads y
    as bf16 and returns dy rounded to bf16, which for a bf16 y loses nothing).  An fp32 y (parity mode) takes the two
    separate ops, so that `forward_loss` equals `forward` + `SimpleLoss` to fp32 accuracy, loss and gradients."""
    if (y.is_cuda and y.dtype == torch.bfloat16 and y.dim() == 4 and y.shape[1] in (64, 128)
            and head.kernel_size == (1, 1) and head.bias is not None
            and head.out_channels in (4, 8) and ytgt.dtype == torch.int64
            and tuple(ytgt.shape) == (y.shape[0], y.shape[2], y.shape[3])):
        return _HeadCEFn.apply(y, head.weight, head.bias, ytgt, weight)
    return weighted_cross_entropy(head(y).float(), ytgt, weight)


class SimpleLoss(torch.nn.Module):
    """ref: src/tools.py:221-231 - weighted 4-class BEV cross-entropy, class weights [1, 10, 5, 10]."""

    def __init__(self, class_weights=(1.0, 10.0, 5.0, 10.0)):
        super().__init__()
        self.register_buffer("weight", torch.tensor(class_weights, dtype=torch.float32), persistent=False)

    def forward(self, ypred, ytgt):
        return weighted_cross_entropy(ypred, ytgt, self.weight.to(ypred.device))


def MultiLoss(bev_pre, act_pre, desc_pre, bev_gt, act_gt, desc_gt, args=None):
    """ref: src/tools.py:234-252 - BEV cross-entropy [1,10,5,10] + weighted BCE-with-logits on the
    action [1,5,5,5] and description [1,5,5,5,1,1,1,1] heads (those two are 4- and 8-element rows:
    library ops)."""
    dev = bev_pre.device
    F = torch.nn.functional
    loss_bev = weighted_cross_entropy(bev_pre, bev_gt, torch.tensor([1.0, 10.0, 5.0, 10.0], device=dev))
    w1 = torch.tensor([1.0, 5.0, 5.0, 5.0], device=dev)
    w2 = torch.tensor([1.0, 5.0, 5.0, 5.0, 1.0, 1.0, 1.0, 1.0], device=dev)
    loss_act = F.binary_cross_entropy_with_logits(act_pre.to(dev), act_gt, weight=w1)
    loss_desc = F.binary_cross_entropy_with_logits(desc_pre.to(dev), desc_gt, weight=w2)
    return loss_bev + loss_act + loss_desc


class ConfusionMatrix(object):
    """ref: src/tools.py:536-585 - running (target, prediction) counts of the segmentation head and the accuracy / IoU
    figures derived from them.  `mat` is None until the first update, then (n, n) int64 on the inputs' device.

    int64 labels on the GPU with n <= 16 are counted by the HIP pass of csrc/metrics.hip (`ops.seg_eval_update*`: two
    launches, no host synchronisation, so `update` can be captured in a HIP graph); everything else takes the
    reference's torch composition (mask, n*a + b, bincount).  `update_from_logits` fuses the argmax - and, given class
    weights, the weighted cross-entropy - into the same read of the logits.

    On the native path a prediction outside [0, n) does not raise inside `update` (that would need a host round trip):
    it is counted on the device and reported by the next host-side read (`compute`, `__str__`,
    `reduce_from_all_processes`)."""

    def __init__(self, num_classes):
        self.num_classes = num_classes
        self.mat = None
        self.loss_acc = None   # (1,) double on the device: sum over batches of batch loss * batch size
        self._invalid = None   # (1,) int64 on the device: out-of-range predictions seen by the native path

    def _ensure(self, device):
        if self.mat is None:
            n = self.num_classes
            self.mat = torch.zeros((n, n), dtype=torch.int64, device=device)
        if self._invalid is None and self.mat.is_cuda:
            self._invalid = torch.zeros(1, dtype=torch.int64, device=self.mat.device)

    def _native(self, *tensors):
        return self.num_classes <= ops.SEG_EVAL_MAXC and all(t.is_cuda and t.numel() > 0 for t in tensors)

    def update(self, a, b):
        """a: targets, b: predicted labels (same number of elements)."""
        self._ensure(a.device)
        with torch.no_grad():
            if self._native(a, b) and a.dtype == torch.int64 and b.dtype == torch.int64:
                ops.seg_eval_update_labels(b.contiguous(), a.contiguous(), self.mat, self._invalid)
                return
            self._update_torch(a, b)

    def _update_torch(self, a, b):
        """The reference's composition: mask, n*a + b, bincount."""
        n = self.num_classes
        keep = (a >= 0) & (a < n)
        pairs = n * a[keep].to(torch.int64) + b[keep]
        self.mat += torch.bincount(pairs, minlength=n ** 2).reshape(n, n)

    def update_from_logits(self, target, logits, class_weight=None):
        """Same counts as `update(target.flatten(), logits.argmax(1).flatten())` from (B, n, ...) logits.  With
        `class_weight` (n floats) it also returns the batch's weighted cross-entropy (targets outside [0, n) carry
        weight 0) as a 0-d tensor on the logits' device and adds loss * B to `loss_acc`, which stays on the device."""
        n = self.num_classes
        self._ensure(logits.device)
        with torch.no_grad():
            w = None
            if class_weight is not None:
                w = torch.as_tensor(class_weight, dtype=torch.float32, device=logits.device).contiguous()
                if self.loss_acc is None:
                    self.loss_acc = torch.zeros(1, dtype=torch.float64, device=logits.device)
            if (self._native(target, logits) and target.dtype == torch.int64 and logits.dim() >= 2
                    and logits.shape[1] == n and logits.dtype in (torch.float32, torch.bfloat16)):
                return ops.seg_eval_update(logits.contiguous(), target.contiguous(), self.mat, w,
                                           None if w is None else self.loss_acc, self._invalid)
            # fp16 / other dtypes, CPU tensors, more than 16 classes: torch ops throughout
            self._update_torch(target.flatten(), logits.argmax(1).flatten())
            if w is None:
                return None
            keep = (target >= 0) & (target < n)
            loss = torch.nn.functional.cross_entropy(logits.float(), torch.where(keep, target, -100).to(torch.int64),
                                                     weight=w)
            self.loss_acc += loss.double() * logits.shape[0]
            return loss

    def total_loss(self):
        """sum over the batches of batch loss * batch size as a Python float (one device read); 0.0 before any."""
        return 0.0 if self.loss_acc is None else float(self.loss_acc.item())

    def reset(self):
        for t in (self.mat, self.loss_acc, self._invalid):
            if t is not None:
                t.zero_()

    def _check_invalid(self):
        if self._invalid is not None:
            bad = int(self._invalid.item())
            if bad:
                raise RuntimeError("ConfusionMatrix(%d): %d predictions outside [0, %d) were passed to update()"
                                   % (self.num_classes, bad, self.num_classes))

    def compute(self):
        """(global accuracy, per-class accuracy, per-class IoU) as fp32 tensors."""
        self._check_invalid()
        h = self.mat.float()
        hit = torch.diag(h)
        acc_global = hit.sum() / h.sum()
        acc = hit / h.sum(1)
        iu = hit / (h.sum(1) + h.sum(0) - hit)
        return acc_global, acc, iu

    def reduce_from_all_processes(self):
        if not torch.distributed.is_available() or not torch.distributed.is_initialized():
            return
        self._check_invalid()
        torch.distributed.barrier()
        torch.distributed.all_reduce(self.mat)
        if self.loss_acc is not None:
            torch.distributed.all_reduce(self.loss_acc)

    def __str__(self):
        acc_global, acc, iu = self.compute()
        pct = lambda t: ['{:.1f}'.format(v) for v in (t * 100).tolist()]  # noqa: E731
        return 'global correct: {:.1f}\naverage row correct: {}\nIoU: {}\nmean IoU: {:.1f}'.format(
            acc_global.item() * 100, pct(acc), pct(iu), iu.mean().item() * 100)


def _progress(loader, use_tqdm):
    if not use_tqdm:
        return loader
    try:
        from tqdm import tqdm
    except ImportError:
        return loader
    return tqdm(loader)


def _to_device(tensors, device):
    return [t.to(device) for t in tensors]


def get_val_info(model, valloader, loss_fn, device, use_tqdm=True):
    """ref: src/tools.py:267-286 - one pass over the validation loader; returns (ConfusionMatrix(4), total_loss) with
    total_loss = sum of batch loss * batch size.  With this package's `SimpleLoss` every batch is ONE fused pass over
    the logits (argmax, counts and weighted cross-entropy) and the loss total is read from the device once, after the
    loop; any other `loss_fn` is called as the reference calls it and only the counts take the fused pass."""
    model.eval()
    confmat = ConfusionMatrix(4)
    fused = isinstance(loss_fn, SimpleLoss)
    total_loss = 0.0
    print('running eval...')
    with torch.no_grad():
        for batch in _progress(valloader, use_tqdm):
            preds = model(*_to_device(batch[:6], device))
            binimgs = batch[6].to(device)
            if fused:
                confmat.update_from_logits(binimgs, preds, loss_fn.weight)
            else:
                total_loss += loss_fn(preds, binimgs).item() * preds.shape[0]
                confmat.update_from_logits(binimgs, preds)
        confmat.reduce_from_all_processes()
        if fused:
            total_loss = confmat.total_loss()
    model.train()
    return confmat, total_loss


def List2List(List):
    """ref: src/tools.py:397-402 - a list of (rows, k) arrays -> the flat row-major list of their elements."""
    import numpy as np
    k = List[0].shape[1]
    return list(np.concatenate([np.asarray(a).reshape(-1, k) for a in List]).ravel())


def _f1_of_label(y_true, y_pred, label):
    """F1 of one label from its true / false positive / negative counts; 0.0 when the denominator is empty."""
    t, p = y_true == label, y_pred == label
    tp = int((t & p).sum())
    denom = 2 * tp + int((~t & p).sum()) + int((t & ~p).sum())
    return 2.0 * tp / denom if denom else 0.0


def f1_binary(y_true, y_pred):
    """sklearn.metrics.f1_score(y_true, y_pred) for 0 / 1 labels: the F1 of label 1 (0.0, silently, when label 1
    occurs nowhere)."""
    import numpy as np
    return _f1_of_label(np.asarray(y_true), np.asarray(y_pred), 1)


def f1_macro(y_true, y_pred):
    """sklearn.metrics.f1_score(y_true, y_pred, average='macro') for 0 / 1 labels: the unweighted mean of the F1 of
    label 0 and of label 1, over the labels that occur in y_true or y_pred (sklearn averages over those only)."""
    import numpy as np
    y_true, y_pred = np.asarray(y_true), np.asarray(y_pred)
    present = [v for v in (0, 1) if (y_true == v).any() or (y_pred == v).any()]
    return float(np.mean([_f1_of_label(y_true, y_pred, v) for v in present]))


def _head_f1(targets, outputs, act_num, desc_num):
    """The six F1 results both multi-head loops return.  targets / outputs: per-batch lists [acts, descs]."""
    import numpy as np
    t_act, t_desc = (np.asarray(List2List(v)) for v in targets)
    o_act, o_desc = (np.asarray(List2List(v)) for v in outputs)
    act_category, desc_category = [0.0] * 4, [0.0] * 8
    for i in range(act_num):
        act_category[i] = f1_binary(t_act[i::act_num], o_act[i::act_num])
    for i in range(desc_num):
        desc_category[i] = f1_binary(t_desc[i::desc_num], o_desc[i::desc_num])
    return (act_category, desc_category, f1_macro(t_act, o_act), f1_macro(t_desc, o_desc),
            np.mean(act_category), np.mean(desc_category))


def _val_heads(model, valloader, device, use_tqdm, act_num, desc_num, confmat):
    """The loop both multi-head validation functions share.  The model returns (bev, act, desc) logits when `confmat`
    is given, (act, desc) otherwise.  The 4- and 8-wide action / description rows stay library ops
    (`sigmoid(x) > 0.5`, which is not `x > 0` in fp32); they are collected on the device and copied to the host once."""
    model.eval()
    print('running eval...')
    acts, descs, acts_gt, descs_gt = [], [], [], []
    with torch.no_grad():
        for batch in _progress(valloader, use_tqdm):
            out = model(*_to_device(batch[:6], device))
            if confmat is not None:
                confmat.update_from_logits(batch[6].to(device), out[0].to(device))
            acts.append(torch.sigmoid(out[-2].to(device)) > 0.5)
            descs.append(torch.sigmoid(out[-1].to(device)) > 0.5)
            acts_gt.append(batch[7])
            descs_gt.append(batch[8])
        if confmat is not None:
            confmat.reduce_from_all_processes()
        n_act = acts[0].shape[1]
        both = torch.cat([torch.cat(acts), torch.cat(descs)], dim=1).cpu().numpy()
        f1 = _head_f1(([g.cpu().numpy() for g in acts_gt], [g.cpu().numpy() for g in descs_gt]),
                      ([both[:, :n_act]], [both[:, n_act:]]), act_num, desc_num)
    model.train()
    return f1


def get_val_info_new(model, valloader, device, use_tqdm=True, act_num=4, desc_num=8):
    """ref: src/tools.py:288-342 - validation of the three-head model: returns (ConfusionMatrix(4), per-action F1 list,
    per-description F1 list, macro F1 over all actions, macro F1 over all descriptions, mean of the action list, mean
    of the description list)."""
    confmat = ConfusionMatrix(4)
    return (confmat,) + _val_heads(model, valloader, device, use_tqdm, act_num, desc_num, confmat)


def get_val_info_nobev(model, valloader, device, use_tqdm=True, act_num=4, desc_num=8):
    """ref: src/tools.py:344-395 - the same for a model without the BEV head: the six F1 results only."""
    return _val_heads(model, valloader, device, use_tqdm, act_num, desc_num, None)
