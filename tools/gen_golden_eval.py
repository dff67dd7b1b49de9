#!/usr/bin/env python3
"""Generate tests/golden/g13_eval.npz by RUNNING THE REFERENCE'S OWN `ConfusionMatrix`, `get_val_info` and
`get_val_info_new` (src/tools.py:267-342, 536-585) on CPU.

Build container only (needs the reference tree, sklearn and tqdm).  The model is a stub `nn.Module` that replays fixed
logits, the loader a list of batches.  `get_val_info` gets `torch.nn.CrossEntropyLoss(weight=[1, 10, 5, 10])`: the
reference's `SimpleLoss` moves its weights to a GPU in its constructor.

Inputs: three batches of (2, 4, 12, 10) logits quantised to multiples of 0.5 (ties occur) with targets that include
-100 and 255, and action / description logits that include 0, 5e-8 and -5e-8 (`sigmoid(5e-8) > 0.5` is False in fp32
although `5e-8 > 0`).  torch's cross-entropy raises on a target of 255, so the `get_val_info` run uses `targets_ce`,
the same targets with 255 replaced by -100; the matrix is the same either way.

Only arrays and strings are stored.

    python tools/gen_golden_eval.py
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from _ref_loader import load_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g13_eval.npz")
NB, B, C, H, W = 3, 2, 4, 12, 10


class Replay(nn.Module):
    """Returns the next recorded output at every call, whatever the inputs."""

    def __init__(self, outputs):
        super().__init__()
        self.outputs, self.calls = outputs, 0

    def forward(self, *inputs):
        out = self.outputs[self.calls % len(self.outputs)]
        self.calls += 1
        return out


def inputs():
    rs = np.random.RandomState(1300)
    logits = (np.round(rs.randn(NB, B, C, H, W) * 3.0) * 0.5).astype(np.float32)
    logits[0, 0, :, 0, 0] = 1.5                       # an all-equal pixel
    logits[1, 1, :, 3, 4] = [0.5, 2.0, 2.0, -1.0]     # a tie for the maximum
    targets = rs.randint(0, C, size=(NB, B, H, W)).astype(np.int64)
    drop = rs.rand(NB, B, H, W)
    targets[drop < 0.10] = -100
    targets[drop > 0.92] = 255
    act = rs.randn(NB, B, 4).astype(np.float32)
    desc = rs.randn(NB, B, 8).astype(np.float32)
    act[:, :, 0] = np.array([0.0, 5e-8, -5e-8, 5e-8, 0.0, -5e-8], np.float32).reshape(NB, B)  # never predicted
    desc[:, :, 1] = np.array([5e-8, 1.0, -5e-8, 0.0, 2.0, 5e-8], np.float32).reshape(NB, B)
    desc[:, :, 7] = -4.0
    acts_gt = (rs.rand(NB, B, 4) < 0.5).astype(np.float32)
    descs_gt = (rs.rand(NB, B, 8) < 0.5).astype(np.float32)
    acts_gt[:, :, 0] = np.array([1, 0, 1, 1, 0, 1], np.float32).reshape(NB, B)
    descs_gt[:, :, 7] = 0.0                            # no positives anywhere: F1 0.0 by definition
    return logits, targets, act, desc, acts_gt, descs_gt


def main():
    rtools, _, _ = load_reference()
    logits, targets, act, desc, acts_gt, descs_gt = inputs()
    targets_ce = np.where(targets == 255, -100, targets)
    tl, tt, tce = torch.from_numpy(logits), torch.from_numpy(targets), torch.from_numpy(targets_ce)
    ta, td = torch.from_numpy(act), torch.from_numpy(desc)
    tag, tdg = torch.from_numpy(acts_gt), torch.from_numpy(descs_gt)
    dummy = [torch.zeros(1)] * 6
    out = dict(logits=logits, targets=targets, targets_ce=targets_ce, act_logits=act, desc_logits=desc,
               acts_gt=acts_gt, descs_gt=descs_gt, class_weights=np.array([1, 10, 5, 10], np.float32))

    cm = rtools.ConfusionMatrix(C)
    for k in range(NB):
        cm.update(tt[k].flatten(), tl[k].argmax(1).flatten())
    acc_global, acc, iu = cm.compute()
    out.update(cm_mat=cm.mat.numpy(), cm_acc_global=acc_global.numpy(), cm_acc=acc.numpy(), cm_iu=iu.numpy(),
               cm_str=np.array(str(cm)))

    model = Replay([tl[k] for k in range(NB)]).train()
    loss_fn = torch.nn.CrossEntropyLoss(weight=torch.tensor([1.0, 10.0, 5.0, 10.0]))
    confmat, total_loss = rtools.get_val_info(model, [tuple(dummy) + (tce[k],) for k in range(NB)], loss_fn, "cpu",
                                              use_tqdm=False)
    assert model.training
    out.update(gvi_mat=confmat.mat.numpy(), gvi_total_loss=np.float64(total_loss), gvi_str=np.array(str(confmat)))

    model = Replay([(tl[k], ta[k], td[k]) for k in range(NB)]).train()
    loader = [tuple(dummy) + (tt[k], tag[k], tdg[k]) for k in range(NB)]
    confmat, act_cat, desc_cat, f1_act, f1_desc, mean_act, mean_desc = rtools.get_val_info_new(
        model, loader, "cpu", use_tqdm=False)
    out.update(gvin_mat=confmat.mat.numpy(), gvin_act_category=np.array(act_cat, np.float64),
               gvin_desc_category=np.array(desc_cat, np.float64), gvin_f1_act=np.float64(f1_act),
               gvin_f1_desc=np.float64(f1_desc), gvin_mean_act=np.float64(mean_act),
               gvin_mean_desc=np.float64(mean_desc))
    np.savez_compressed(OUT, **out)
    for k in ("cm_mat", "cm_str", "gvi_total_loss", "gvin_act_category", "gvin_desc_category", "gvin_f1_act",
              "gvin_f1_desc"):
        print(k, out[k])
    print("wrote", OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
