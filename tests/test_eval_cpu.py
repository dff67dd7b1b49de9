"""The validation path without a GPU: `ConfusionMatrix`, `get_val_info`, `get_val_info_new` on CPU tensors against the
outputs the reference's own functions recorded in tests/golden/g13_eval.npz (tools/gen_golden_eval.py), the numpy F1
helpers, the argument checks of the new C entry points, and `reduce_from_all_processes` over two gloo ranks."""
import ctypes
import os
import socket
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import lss2_multimodal_nu_amd as L
from lss2_multimodal_nu_amd import tools as T


class Replay(torch.nn.Module):
    """Stub model: returns the next recorded output at every call and notes the state it was called in."""

    def __init__(self, outputs):
        super().__init__()
        self.outputs, self.calls, self.seen = outputs, 0, []

    def forward(self, *inputs):
        self.seen.append((self.training, torch.is_grad_enabled(), len(inputs)))
        out = self.outputs[self.calls % len(self.outputs)]
        self.calls += 1
        return out


def _batches(g, targets="targets", heads=False):
    dummy = (torch.zeros(1),) * 6
    nb = g["logits"].shape[0]
    t = torch.from_numpy(g[targets])
    if not heads:
        return [dummy + (t[k],) for k in range(nb)]
    ag, dg = torch.from_numpy(g["acts_gt"]), torch.from_numpy(g["descs_gt"])
    return [dummy + (t[k], ag[k], dg[k]) for k in range(nb)]


@pytest.fixture(scope="module")
def g13(golden):
    return golden("g13_eval")


def test_confusion_matrix_reproduces_the_reference(g13):
    logits, targets = torch.from_numpy(g13["logits"]), torch.from_numpy(g13["targets"])
    cm = L.ConfusionMatrix(4)
    assert cm.num_classes == 4 and cm.mat is None
    for k in range(logits.shape[0]):
        cm.update(targets[k].flatten(), logits[k].argmax(1).flatten())
    assert cm.mat.dtype == torch.int64 and tuple(cm.mat.shape) == (4, 4)
    assert np.array_equal(cm.mat.numpy(), g13["cm_mat"])
    acc_global, acc, iu = cm.compute()
    assert acc_global.dtype == torch.float32
    assert np.array_equal(acc_global.numpy(), g13["cm_acc_global"])
    assert np.array_equal(acc.numpy(), g13["cm_acc"])
    assert np.array_equal(iu.numpy(), g13["cm_iu"])
    assert str(cm) == str(g13["cm_str"])
    # the fused form gives the same counts
    cm2 = L.ConfusionMatrix(4)
    for k in range(logits.shape[0]):
        assert cm2.update_from_logits(targets[k], logits[k]) is None
    assert torch.equal(cm2.mat, cm.mat)
    cm.reset()
    assert int(cm.mat.sum()) == 0


def test_get_val_info_reproduces_the_reference(g13):
    model = Replay([torch.from_numpy(g13["logits"][k]) for k in range(3)]).train()
    loss_fn = torch.nn.CrossEntropyLoss(weight=torch.from_numpy(g13["class_weights"]))
    confmat, total_loss = L.get_val_info(model, _batches(g13, "targets_ce"), loss_fn, "cpu", use_tqdm=False)
    assert np.array_equal(confmat.mat.numpy(), g13["gvi_mat"])
    assert str(confmat) == str(g13["gvi_str"])
    assert isinstance(total_loss, float)
    assert total_loss == float(g13["gvi_total_loss"])   # same CPU ops in the same order: bit-equal, not just 1e-6
    # eval mode and no_grad inside the loop, six inputs per call, train mode again afterwards
    assert model.seen == [(False, False, 6)] * 3 and model.training


def test_get_val_info_with_simple_loss_ignores_out_of_range_targets(g13):
    """`SimpleLoss` takes the fused form (on CPU tensors: its torch composition), where 255 is ignored like -100."""
    model = Replay([torch.from_numpy(g13["logits"][k]) for k in range(3)])
    confmat, total_loss = L.get_val_info(model, _batches(g13), L.SimpleLoss(), "cpu", use_tqdm=False)
    assert np.array_equal(confmat.mat.numpy(), g13["gvi_mat"])
    assert total_loss == pytest.approx(float(g13["gvi_total_loss"]), rel=1e-6)
    assert model.seen == [(False, False, 6)] * 3 and model.training


def test_get_val_info_new_reproduces_the_reference(g13):
    outs = [(torch.from_numpy(g13["logits"][k]), torch.from_numpy(g13["act_logits"][k]),
             torch.from_numpy(g13["desc_logits"][k])) for k in range(3)]
    model = Replay(outs).train()
    got = L.get_val_info_new(model, _batches(g13, heads=True), "cpu", use_tqdm=True)
    assert len(got) == 7
    confmat, act_cat, desc_cat, f1_act, f1_desc, mean_act, mean_desc = got
    assert np.array_equal(confmat.mat.numpy(), g13["gvin_mat"])
    assert isinstance(act_cat, list) and isinstance(desc_cat, list)
    assert np.array_equal(np.array(act_cat), g13["gvin_act_category"])
    assert np.array_equal(np.array(desc_cat), g13["gvin_desc_category"])
    assert (f1_act, f1_desc) == (float(g13["gvin_f1_act"]), float(g13["gvin_f1_desc"]))
    assert (mean_act, mean_desc) == (float(g13["gvin_mean_act"]), float(g13["gvin_mean_desc"]))
    assert act_cat[0] == 0.0     # logits 0 / 5e-8 / -5e-8: sigmoid(x) > 0.5 never fires, x > 0 would
    assert model.seen == [(False, False, 6)] * 3 and model.training
    # the two-head form: the same six F1 results, no matrix
    model2 = Replay([o[1:] for o in outs]).train()
    got2 = L.get_val_info_nobev(model2, _batches(g13, heads=True), "cpu", use_tqdm=False)
    assert len(got2) == 6 and got2[0] == act_cat and got2[1] == desc_cat and got2[2:] == got[3:]
    assert model2.seen == [(False, False, 6)] * 3 and model2.training


def test_list2list_is_the_row_major_flattening():
    a = [np.arange(6).reshape(2, 3), np.arange(6, 12).reshape(2, 3), np.arange(12, 15).reshape(1, 3)]
    out = L.List2List(a)
    assert isinstance(out, list) and [int(v) for v in out] == list(range(15))


def test_f1_hand_computed():
    t = np.array([1, 1, 1, 0, 0, 0, 0, 1])
    p = np.array([1, 1, 0, 0, 0, 1, 0, 0])
    # label 1: tp 2, fp 1, fn 2 -> 4 / 7;  label 0: tp 3, fp 2, fn 1 -> 6 / 9
    assert T.f1_binary(t, p) == 4.0 / 7.0
    assert T.f1_macro(t, p) == pytest.approx((4.0 / 7.0 + 6.0 / 9.0) / 2, abs=1e-15)
    assert T.f1_binary(t.astype(np.float32), p.astype(bool)) == 4.0 / 7.0
    zeros = np.zeros(5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")        # the empty denominator is 0.0 without a warning
        assert T.f1_binary(zeros, zeros) == 0.0
        assert T.f1_binary(np.ones(5), zeros) == 0.0
        assert T.f1_macro(zeros, zeros) == 1.0   # only label 0 occurs, and it is always right
        assert T.f1_macro(np.ones(4), np.zeros(4)) == 0.0
    assert T.f1_binary(np.ones(3), np.ones(3)) == 1.0


def test_f1_equals_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    rs = np.random.RandomState(5)
    cases = [((rs.rand(n) < pt).astype(np.float32), rs.rand(n) < pp)
             for n, pt, pp in ((1, 0.5, 0.5), (7, 0.5, 0.5), (64, 0.1, 0.9), (257, 0.3, 0.3), (40, 0.0, 0.5),
                               (40, 0.5, 0.0), (40, 0.0, 0.0), (40, 1.0, 1.0), (40, 1.0, 0.0))]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for t, p in cases:
            assert abs(T.f1_binary(t, p) - metrics.f1_score(t, p)) <= 1e-12
            assert abs(T.f1_macro(t, p) - metrics.f1_score(t, p, average="macro")) <= 1e-12


def test_package_does_not_import_sklearn():
    import re
    assert not re.search(r"^\s*(from|import)\s+sklearn", open(T.__file__).read(), flags=re.M)


def test_seg_eval_abi_argument_checks():
    """Every check of the new entry points happens before any HIP call."""
    from lss2_multimodal_nu_amd import _native
    lib = _native.lib()
    need = lib.lss_seg_eval_workspace_bytes
    assert need(4) > 0 and need(1) > 0 and need(16) > need(4)
    assert need(17) == 0 and need(0) == 0
    one, odd, big = ctypes.c_void_p(64), ctypes.c_void_p(66), 1 << 20
    up, lab = lib.lss_seg_eval_update, lib.lss_seg_eval_update_labels
    # logits, dtype, target, class_weight, B, C, HW, workspace, workspace_bytes, confmat, batch_loss, loss_acc, stream
    assert up(None, 0, one, None, 1, 4, 16, one, big, one, None, None, None) == -1      # LSS_E_NULL
    assert up(one, 0, None, None, 1, 4, 16, one, big, one, None, None, None) == -1
    assert up(one, 0, one, None, 1, 4, 16, None, big, one, None, None, None) == -1
    assert up(one, 0, one, None, 1, 4, 16, one, big, None, None, None, None) == -1
    assert up(one, 0, one, one, 1, 4, 16, one, big, one, None, None, None) == -1        # weights without batch_loss
    assert up(one, 0, one, None, 1, 0, 16, one, big, one, None, None, None) == -2       # LSS_E_SHAPE: C = 0
    assert up(one, 0, one, None, 1, 17, 16, one, big, one, None, None, None) == -2      # C = 17
    assert up(one, 0, one, None, 1, 4, 0, one, big, one, None, None, None) == -2        # HW = 0
    assert up(one, 0, one, None, 0, 4, 16, one, big, one, None, None, None) == -2       # B = 0
    assert up(one, 0, one, None, 2, 4, 1 << 30, one, big, one, None, None, None) == -2  # B*HW = 2^31
    assert up(one, 0, one, None, 1, 4, 1 << 31, one, big, one, None, None, None) == -2
    assert up(one, 2, one, None, 1, 4, 16, one, big, one, None, None, None) == -3       # LSS_E_LAYOUT
    assert up(one, -1, one, None, 1, 4, 16, one, big, one, None, None, None) == -3
    assert up(odd, 0, one, None, 1, 4, 16, one, big, one, None, None, None) == -4       # LSS_E_ALIGN: fp32 at 2 mod 4
    assert up(one, 1, odd, None, 1, 4, 16, one, big, one, None, None, None) == -4
    assert up(one, 0, one, None, 1, 4, 16, one, need(4) - 1, one, None, None, None) == -5   # LSS_E_WORKSPACE
    assert up(one, 0, one, None, 1, 16, 16, one, need(4), one, None, None, None) == -5
    # pred, target, n, C, workspace, workspace_bytes, confmat, invalid, stream
    assert lab(None, one, 16, 4, one, big, one, one, None) == -1
    assert lab(one, one, 16, 4, one, big, one, None, None) == -1
    assert lab(one, one, 16, 0, one, big, one, one, None) == -2
    assert lab(one, one, 16, 17, one, big, one, one, None) == -2
    assert lab(one, one, 0, 4, one, big, one, one, None) == -2
    assert lab(one, one, 1 << 31, 4, one, big, one, one, None) == -2
    assert lab(odd, one, 16, 4, one, big, one, one, None) == -4
    assert lab(one, one, 16, 4, one, 8, one, one, None) == -5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_eval.npz"))
    logits, targets = torch.from_numpy(g["logits"]), torch.from_numpy(g["targets"])
    cm = L.ConfusionMatrix(4)
    for k in range(logits.shape[0]):      # each rank takes one sample of every batch
        cm.update_from_logits(targets[k, rank:rank + 1], logits[k, rank:rank + 1], g["class_weights"])
    local = cm.mat.clone()
    cm.reduce_from_all_processes()
    torch.save({"mat": cm.mat, "local": local, "loss_acc": cm.loss_acc}, "%s.%d" % (out, rank))
    dist.destroy_process_group()


def test_two_gloo_ranks_reduce_to_the_single_process_matrix(tmp_path, g13):
    out = str(tmp_path / "cm.pt")
    mp.spawn(_rank, args=(2, _free_port(), out), nprocs=2, join=True)
    got = [torch.load("%s.%d" % (out, r)) for r in range(2)]
    want = torch.from_numpy(g13["cm_mat"])
    for r in range(2):
        assert torch.equal(got[r]["mat"], want)
        assert not torch.equal(got[r]["local"], want)
    assert torch.equal(got[0]["local"] + got[1]["local"], want)
    assert torch.equal(got[0]["loss_acc"], got[1]["loss_acc"]) and float(got[0]["loss_acc"]) > 0


def test_reduce_is_a_no_op_without_a_process_group():
    cm = L.ConfusionMatrix(3)
    cm.update(torch.tensor([0, 1, 2, 2, -100]), torch.tensor([0, 2, 2, 2, 1]))
    before = cm.mat.clone()
    cm.reduce_from_all_processes()
    assert torch.equal(cm.mat, before) and cm.mat.tolist() == [[1, 0, 0], [0, 0, 1], [0, 0, 2]]


def test_more_than_16_classes_take_the_torch_composition():
    torch.manual_seed(3)
    x, t = torch.randn(2, 17, 5, 3), torch.randint(-1, 18, (2, 5, 3))
    cm = L.ConfusionMatrix(17)
    loss = cm.update_from_logits(t, x, torch.ones(17))
    keep = (t >= 0) & (t < 17)
    want = torch.bincount(17 * t[keep] + x.argmax(1)[keep], minlength=289).reshape(17, 17)
    assert torch.equal(cm.mat, want)
    ref = torch.nn.functional.cross_entropy(x, torch.where(keep, t, -100))
    assert float(loss) == pytest.approx(float(ref), rel=1e-6)
    assert cm.total_loss() == pytest.approx(float(ref) * 2, rel=1e-6)
