"""Drop-in for the reference's `src/model_vovnet_transformer.py`: the depth heads
(`MultiScaleDepthNet` :22-70, `StandardDepthNet` :73-87), `CamEncodeV2` :90-122,
`BEVEncoderTransformer` :125-173, the TXT-branch blocks :176-351 and
`VoVNetBEVTransformer` :354-639 with its factory :642-688.

Same constructor arguments, `forward()` signatures, public methods
(`create_frustum`, `get_geometry`, `voxel_pooling`) and `state_dict` keys.  The
camera->BEV half runs on the HIP kernels of csrc/ (C = 128 context channels):

    K3 points->voxels   ||  3x3 depth-head convs (K8, MFMA)
                            K2v 1x1 depth logits + feat_proj (+ softmax for v1)
                            [v2: fusion of the two scales + softmax]
                        ->  K4 bucket  ->  K5 fused lift-splat

What is NOT here: the VoVNet trunk (`timm`, third-party weights, a by-name
network fetch in the reference, src/vovnet_timm.py:48-53).  `backbone=` accepts
any module returning {'c3': (B*N,768,H/16,W/16), 'c4': (B*N,1024,H/32,W/32)};
the default passes such feature maps straight through.

The TXT branch: c3 -> feature pyramid -> ASPP -> per-camera scene tokens is about a seventh of the step's FLOPs and
runs at inference on K13 (csrc/camera_branch.hip, `VoVNetBEVTransformer.scene_tokens`); the six-token tail behind it
(camera transformer, BEV fusion, predictor) and the pooled BEV token run at inference on K14 (csrc/camera_tail.hip, two
launches) and are stock PyTorch everywhere else.
"""
import os

import torch
from torch import nn
from torch.autograd.function import once_differentiable
from torch.nn import functional as F

from . import modules, ops
from .heads import SceneUnder
from .model_BEV_TXT import _LiftSplatMixin, _histogram_guard
from .modules import _FoldedConv, _PRECISIONS, _bn_is, _conv_is, _needs_autograd, _to_nhwc, default_precision
from .tools import QuickCumsum, gen_dx_bx  # noqa: F401  (reference's import surface)
from .tools import head_1x1, head_weighted_cross_entropy, weighted_cross_entropy
from .transformer_modules import LightweightBEVTransformer


# ----------------------------------------------------------------------------
# Autograd nodes of the lift-splat level (training): the 1x1 heads and the splat run on the inference kernels, their
# backward on K7 + K10; the lifted (B,N,D,fH,fW,C) tensor exists in neither direction.
# ----------------------------------------------------------------------------
LIFT_CALLS = {"native": 0, "composition": 0}  # which form `get_voxels` took when it had to be differentiable
# which form BEVEncoderTransformer.forward / forward_loss took when it had to be differentiable: "native" = the 1x1
# compress unit, the two biased 3x3 units and the 64-channel head on the HIP kernels (bf16 autocast)
BEV_ENCODER_CALLS = {"native": 0, "composition": 0}
# LSS_BEV_ENCODER_NATIVE unset: see DESIGN.md 4b for the measurement that decides this
_BEV_ENCODER_NATIVE_DEFAULT = "1"


# which form each 3x3 conv-BN-ReLU unit of the depth heads / v2's fusion tail took when `get_voxels` had to be
# differentiable: "native" = `modules._train_conv_bn_act` with the bias absorbed (bf16 autocast) / `_DepthFuseFn`
HEAD_UNIT_CALLS = {"native": 0, "composition": 0}
FUSE_TAIL_CALLS = {"native": 0, "composition": 0}
# LSS_DEPTH_HEADS_NATIVE / LSS_DEPTH_TAIL_NATIVE unset: see DESIGN.md 4b for the measurements that decide these
_DEPTH_HEADS_NATIVE_DEFAULT = "1"
_DEPTH_TAIL_NATIVE_DEFAULT = "1"
# which form `VoVNetBEVTransformer.scene_tokens` took: "native" = K13 (eval, no autograd, bf16, GPU), "composition" =
# sceneunder(feature_pyramid(c3)).mean((2, 3)) on library ops
CAMERA_BRANCH_CALLS = {"native": 0, "composition": 0}
# LSS_CAMERA_BRANCH_NATIVE unset: see DESIGN.md 4b for the measurement that decides this
_CAMERA_BRANCH_NATIVE_DEFAULT = "1"
# which form a TRAINING call of `scene_tokens` took (a module in training mode, or gradients wanted): "native" = the
# conv-BN autograd units on the HIP kernels (bf16 autocast, GPU, K16 for the dilated weight gradients), "composition" =
# the library ops.  CAMERA_BRANCH_CALLS counts the composition as before and does not count the native training form.
CAMERA_BRANCH_TRAIN_CALLS = {"native": 0, "composition": 0}
# LSS_CAMERA_BRANCH_TRAIN_NATIVE unset: see DESIGN.md 4b for the measurement that decides this
_CAMERA_BRANCH_TRAIN_NATIVE_DEFAULT = "1"


class _MapLike:
    """Stand-in for a GPU (B, C, H, W) map that does not exist yet: what the training units' guards read of a tensor."""
    is_cuda = True

    def __init__(self, *shape):
        self.shape = tuple(shape)

    def dim(self):
        return len(self.shape)
# which form the six-token tail of `VoVNetBEVTransformer.forward` took on the inference branch: "native" = K14 (bev_pool +
# camera_tail: eval, no autograd, fp32 parameters, GPU, no forward hooks), "composition" = the pooled map through
# camera_transformer, bev_fusion and unified_predictor on library ops
CAMERA_TAIL_CALLS = {"native": 0, "composition": 0}
# LSS_CAMERA_TAIL_NATIVE unset: see DESIGN.md 4b for the measurement that decides this
_CAMERA_TAIL_NATIVE_DEFAULT = "1"


def _nhwc_bf16_rows(hidden):
    """The (BN,fH,fW,Cd) bf16 rows behind `hidden` when it is a bf16 NCHW view over contiguous NHWC memory (what the
    native 3x3 unit returns), else None."""
    if hidden.dtype != torch.bfloat16 or hidden.dim() != 4:
        return None
    rows = hidden.permute(0, 2, 3, 1)
    return rows if rows.is_contiguous() else None


class _HeadProjFn(torch.autograd.Function):
    """The 1x1 convs behind the depth heads' hidden map (BN,Cd,fH,fW) and (optionally, same launch) `feat_proj`
    over C3.
    forward = K2v without softmax, fp32 math: logits (BN,D,fH,fW) [, context rows (BN,fH,fW,C)];
    backward = K10 once per projection, reading the gradients where K7 left them.
    A hidden map that arrives as a bf16 NCHW view over NHWC memory (the native 3x3 unit's output) is read where it
    lies in both directions - K2v takes bf16 rows, K10 has a bf16 NHWC mode - and its gradient goes back the same
    way; an fp32 NCHW map takes the fp32 copies."""

    @staticmethod
    def forward(ctx, hidden, w_depth, b_depth, c3, w_feat, b_feat):
        # (no `custom_fwd(cast_inputs=...)`: it would turn the bf16 rows into an fp32 copy; the casts it would make
        # are made here, for everything else)
        rows16 = _nhwc_bf16_rows(hidden)
        with torch.autocast("cuda", enabled=False):
            w_depth, b_depth = w_depth.float(), b_depth.float()
            if c3 is not None:
                c3, w_feat, b_feat = c3.float(), w_feat.float(), b_feat.float()
            if rows16 is None:
                hidden = hidden.float()
            return _HeadProjFn._forward(ctx, hidden, rows16, w_depth, b_depth, c3, w_feat, b_feat)

    @staticmethod
    def _forward(ctx, hidden, rows16, w_depth, b_depth, c3, w_feat, b_feat):
        ctx.nhwc = rows16 is not None
        if ctx.nhwc:
            hidden = rows = rows16  # kept for K10 as it lies
        else:
            hidden = hidden.contiguous()  # (BN,Cd,fH,fW): kept for K10 as it is (the tensor the ReLU's backward holds)
            rows = hidden.permute(0, 2, 3, 1).contiguous()  # the NHWC rows K2v reads; freed when the node returns
        with_feat = c3 is not None
        if with_feat:
            c3 = c3.contiguous()
        logits, feat = ops.camencode_v2(rows, w_depth.contiguous(), b_depth.contiguous(), w_depth.shape[0], c3,
                                        w_feat.contiguous() if with_feat else None,
                                        b_feat.contiguous() if with_feat else None, softmax=False, math=ops.DT_F32)
        ctx.save_for_backward(hidden, w_depth, c3, w_feat)
        ctx.with_feat = with_feat
        return (logits, feat) if with_feat else logits

    @staticmethod
    @once_differentiable
    def backward(ctx, g_logits, g_feat=None):
        with torch.autocast("cuda", enabled=False):
            return _HeadProjFn._backward(ctx, g_logits, g_feat)

    @staticmethod
    def _backward(ctx, g_logits, g_feat):
        hidden, w_depth, c3, w_feat = ctx.saved_tensors
        need = ctx.needs_input_grad
        out = [None] * 6
        if need[0] or need[1] or need[2]:
            out[0], out[1], out[2] = ops.pointwise_conv_bwd(g_logits, hidden, w_depth.contiguous(),
                                                            layout="nhwc" if ctx.nhwc else "nchw",
                                                            want_dx=need[0], want_dw=need[1], want_db=need[2])
            if ctx.nhwc and out[0] is not None:
                out[0] = out[0].permute(0, 3, 1, 2)  # bf16 NHWC dx, handed back as the NCHW view it came as
        if ctx.with_feat and (need[3] or need[4] or need[5]):
            # (BN,fH,fW,C) rows as autograd sees them; K7 wrote them channel-major, and that is how K10 reads them
            out[3], out[4], out[5] = ops.pointwise_conv_bwd(g_feat.permute(0, 3, 1, 2), c3, w_feat.contiguous(),
                                                            layout="nchw", want_dx=need[3], want_dw=need[4],
                                                            want_db=need[5])
        return tuple(out)


class _HeadsLiftSplatFn(torch.autograd.Function):
    """(pre-softmax depth map u (BN,D,fH,fW), context rows (BN,fH,fW,C), calibration) -> BEV grid.  forward = softmax
    over D + `lift_splat_from_heads` (K3 / K4 / K5 behind one native call); backward = K7, which applies the softmax
    backward itself and returns both gradients in one (BN, D + C, fH, fW) tensor: they are handed on as views of it."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, u, feat, calib, consts, ws, dims, nx, layout):
        inv_pr, comb, ptr, trn = calib
        frustum, dx, bx = consts
        depth = torch.softmax(u, dim=1)
        feat = feat.contiguous()
        with _histogram_guard(ws):  # a failed call must not leave the zero-between-calls words of the workspace dirty
            bev = ops.lift_splat_from_heads(frustum, inv_pr, ptr, comb, trn, dx, bx, depth, feat, ws, dims, nx, layout)
        ctx.save_for_backward(depth, feat, ws.voxel.clone())
        ctx.dims, ctx.nx = dims, nx
        return bev

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_bev):
        depth, feat, voxel = ctx.saved_tensors
        D = ctx.dims[2]
        g = ops.lift_splat_bwd(grad_bev, voxel, depth, feat, ctx.dims, ctx.nx)  # (BN, D + C, fH, fW)
        return g[:, :D], g[:, D:].permute(0, 2, 3, 1), None, None, None, None, None, None


class _DepthFuseFn(torch.autograd.Function):
    """v2's fusion tail in training mode as one node (csrc/depth_fuse_train.hip): (d3 (BN,D,H,W), d4 (BN,D,H4,W4)
    logits) -> relu(BatchNorm_train(fusion([d3, bilinear(d4)]))) (BN,D,H,W), the softmax's input.  fp32 math, three
    launches forward and four backward; the upsampled and the concatenated tensor exist in neither direction.  The
    conv bias stays in the pre-activation (running_mean is the biased conv's), its gradient is the exact zero it is
    in exact arithmetic (`modules._AbsorbedBiasFn`'s convention)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, d3, d4, weight, bias, gamma, beta, running_mean, running_var, momentum, eps):
        d3, d4 = d3.contiguous(), d4.contiguous()
        w, g32 = weight.detach().contiguous(), gamma.detach().contiguous()
        z, u, mean, invstd = ops.depth_fuse_train_fwd(d3, d4, w, bias.detach().contiguous(), g32,
                                                      beta.detach().contiguous(), running_mean, running_var, momentum,
                                                      eps)
        ctx.save_for_backward(d3, d4, w, g32, z, u, mean, invstd)
        ctx.bias_meta = (bias.shape, bias.dtype)
        return u

    @staticmethod
    @once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, du):
        d3, d4, w, g32, z, u, mean, invstd = ctx.saved_tensors
        if du.dtype != torch.float32:
            du = du.float()
        dd3, dd4, dw, dgamma, dbeta = ops.depth_fuse_train_bwd(du.contiguous(), u, z, d3, d4, w, g32, mean, invstd)
        need = ctx.needs_input_grad
        shape, dtype = ctx.bias_meta
        db = torch.zeros(shape, dtype=dtype, device=du.device) if need[3] else None
        return (dd3 if need[0] else None, dd4 if need[1] else None, dw if need[2] else None, db,
                dgamma if need[4] else None, dbeta if need[5] else None, None, None, None, None)


def _fuse_tail_native_ok(fusion, d3):
    """Does v2's fusion tail take `_DepthFuseFn`?  (The caller is on the lift's native route already - GPU tensors,
    fp32 modules.)  A plain 1x1 conv 2D -> D with D <= 64 and a bias, and a BatchNorm in training mode that is affine,
    tracks running statistics with a numeric momentum, is fp32 and is not synchronised over ranks; LSS_DEPTH_TAIL_NATIVE=0
    keeps the torch composition.  With or without autocast: the node's math is fp32 either way."""
    if os.environ.get("LSS_DEPTH_TAIL_NATIVE", _DEPTH_TAIL_NATIVE_DEFAULT) == "0":
        return False
    conv, bn = fusion[0], fusion[1]
    D = conv.out_channels
    if not (isinstance(conv, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d) and d3.is_cuda and d3.dim() == 4):
        return False
    if not (bn.training and bn.affine and bn.track_running_stats and bn.momentum is not None
            and bn.weight.dtype == torch.float32 and bn.num_features == D and "_lss_sync" not in bn.__dict__):
        return False
    return (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.bias is not None and conv.in_channels == 2 * D and D <= 64
            and d3.shape[1] == D and conv.weight.dtype == torch.float32
            and d3.shape[0] * d3.shape[2] * d3.shape[3] < 2 ** 31)


def _head_hidden(head, c):
    """The 3x3 conv-BN-ReLU in front of a depth head's 1x1 on the autograd path: the bias-absorbing HIP unit under bf16
    autocast (`modules._biased_conv3x3_unit_ok`; LSS_DEPTH_HEADS_NATIVE=0 switches it off), else the stock modules."""
    if (os.environ.get("LSS_DEPTH_HEADS_NATIVE", _DEPTH_HEADS_NATIVE_DEFAULT) != "0"
            and modules._biased_conv3x3_unit_ok(head[0], head[1], c.is_cuda, c.shape[1])):
        HEAD_UNIT_CALLS["native"] += 1
        return modules._train_conv_bn_act(head[0], head[1], c, relu=True)
    HEAD_UNIT_CALLS["composition"] += 1
    return head[2](head[1](head[0](c)))


def _fuse_tail(fusion, d3, d4):
    """v2's tail on the autograd path: relu(bn(conv1x1(cat([d3, bilinear(d4)])))), the softmax's input - `_DepthFuseFn`
    where `_fuse_tail_native_ok` holds, the five torch ops otherwise."""
    if _fuse_tail_native_ok(fusion, d3):
        FUSE_TAIL_CALLS["native"] += 1
        conv, bn = fusion[0], fusion[1]
        u = _DepthFuseFn.apply(d3, d4, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                               float(bn.momentum), float(bn.eps))
        modules._count_batch(bn)
        return u
    FUSE_TAIL_CALLS["composition"] += 1
    d4 = F.interpolate(d4, size=d3.shape[2:], mode="bilinear", align_corners=False)
    return fusion(torch.cat([d3, d4], dim=1))


def _conv_bn_relu_head(cin, D):
    return nn.Sequential(nn.Conv2d(cin, 256, 3, padding=1), nn.BatchNorm2d(256), nn.ReLU(inplace=True),
                         nn.Conv2d(256, D, 1))


def _dt(precision):
    return _PRECISIONS[precision or default_precision()]


class StandardDepthNet(nn.Module):
    """Single-scale depth head: 3x3 conv-BN-ReLU, 1x1 conv, softmax over depth bins."""

    def __init__(self, c3_channels=768, depth_channels=41, precision=None):
        super().__init__()
        self.depth_head = _conv_bn_relu_head(c3_channels, depth_channels)
        self.precision = precision
        self._f = _FoldedConv(self.depth_head[0], self.depth_head[1])

    def hidden(self, c3):
        """(BN, fH, fW, 256) NHWC activations of the 3x3 conv-BN-ReLU (K8)."""
        dt = _dt(self.precision)
        return self._f.run(_to_nhwc(c3, dt), dt, relu=True)

    def depth_and_context(self, c3, c4, cam_encode):
        """One K2v launch: softmax depth (BN,D,fH,fW) + context rows (BN,fH,fW,C)."""
        last = self.depth_head[3]
        return ops.camencode_v2(self.hidden(c3), last.weight.detach(), last.bias.detach(), last.out_channels,
                                c3.float().contiguous(), cam_encode.feat_proj.weight.detach(),
                                cam_encode.feat_proj.bias.detach())

    def pre_softmax_and_context(self, c3, c4, cam_encode):
        """Differentiable: logits (BN,D,fH,fW) + context rows (BN,fH,fW,C); the 3x3 conv-BN-ReLU is the HIP unit with
        the bias absorbed under bf16 autocast and torch autograd otherwise (`_head_hidden`), the two 1x1 convs are one
        `_HeadProjFn` node."""
        last, fp = self.depth_head[3], cam_encode.feat_proj
        h = _head_hidden(self.depth_head, c3)
        return _HeadProjFn.apply(h, last.weight, last.bias, c3, fp.weight, fp.bias)

    def forward(self, c3, c4=None):
        if _needs_autograd(self, c3):
            return F.softmax(self.depth_head(c3), dim=1)
        last = self.depth_head[3]
        depth, _ = ops.camencode_v2(self.hidden(c3), last.weight.detach(), last.bias.detach(), last.out_channels)
        return depth


class MultiScaleDepthNet(nn.Module):
    """Depth logits from C3 (1/16) and C4 (1/32); the coarse logits are bilinearly
    upsampled (align_corners=False), concatenated, fused by 1x1 conv-BN-ReLU, softmax."""

    def __init__(self, c3_channels=768, c4_channels=1024, depth_channels=41, precision=None):
        super().__init__()
        D = depth_channels
        self.depth_c3 = _conv_bn_relu_head(c3_channels, D)
        self.depth_c4 = _conv_bn_relu_head(c4_channels, D)
        self.fusion = nn.Sequential(nn.Conv2d(D * 2, D, 1), nn.BatchNorm2d(D), nn.ReLU(inplace=True))
        self.precision = precision
        self._f3 = _FoldedConv(self.depth_c3[0], self.depth_c3[1])
        self._f4 = _FoldedConv(self.depth_c4[0], self.depth_c4[1])
        self._ff = _FoldedConv(self.fusion[0], self.fusion[1], pack=False)

    def _fuse(self, d3, d4):
        _, scale, shift = self._ff.get(ops.DT_F32)
        return ops.depth_fuse_softmax(d3, d4, self.fusion[0].weight.detach(), scale, shift)

    def depth_and_context(self, c3, c4, cam_encode):
        dt = _dt(self.precision)
        D = self.fusion[0].out_channels
        h3 = self._f3.run(_to_nhwc(c3, dt), dt, relu=True)
        h4 = self._f4.run(_to_nhwc(c4, dt), dt, relu=True)
        l3, l4 = self.depth_c3[3], self.depth_c4[3]
        fp = None if cam_encode is None else cam_encode.feat_proj
        d3, feat = ops.camencode_v2(h3, l3.weight.detach(), l3.bias.detach(), D,
                                    None if fp is None else c3.float().contiguous(),
                                    None if fp is None else fp.weight.detach(),
                                    None if fp is None else fp.bias.detach(), softmax=False)
        d4, _ = ops.camencode_v2(h4, l4.weight.detach(), l4.bias.detach(), D, softmax=False)
        return self._fuse(d3, d4), feat

    def pre_softmax_and_context(self, c3, c4, cam_encode):
        """Differentiable: the fusion conv-BN-ReLU output (the softmax's input) + context rows.  The 3x3 conv-BN-ReLU
        units are the HIP units with the bias absorbed under bf16 autocast (`_head_hidden`), the three 1x1 projections
        two `_HeadProjFn` nodes, and the tail - bilinear upsample of the C4 logits, concat, fusion conv, train-mode
        BatchNorm, ReLU - one `_DepthFuseFn` node (`_fuse_tail_native_ok`); otherwise torch autograd."""
        l3, l4, fp = self.depth_c3[3], self.depth_c4[3], cam_encode.feat_proj
        h3 = _head_hidden(self.depth_c3, c3)
        h4 = _head_hidden(self.depth_c4, c4)
        d3, feat = _HeadProjFn.apply(h3, l3.weight, l3.bias, c3, fp.weight, fp.bias)
        d4 = _HeadProjFn.apply(h4, l4.weight, l4.bias, None, None, None)
        return _fuse_tail(self.fusion, d3, d4), feat

    def forward(self, c3, c4):
        if _needs_autograd(self, c3, c4):
            d3 = self.depth_c3(c3)
            d4 = F.interpolate(self.depth_c4(c4), size=d3.shape[2:], mode="bilinear", align_corners=False)
            return F.softmax(self.fusion(torch.cat([d3, d4], dim=1)), dim=1)
        return self.depth_and_context(c3, c4, None)[0]


class CamEncodeV2(nn.Module):
    """feat_proj 1x1 conv, then depth (x) context outer product.  `forward`
    materialises the (B*N, C_out, D, H, W) lifted tensor only because that is its
    return value; the fused model path never forms it."""

    def __init__(self, D, C_in, C_out):
        super().__init__()
        self.D = D
        self.C_out = C_out
        self.feat_proj = nn.Conv2d(C_in, C_out, 1)
        self._f = _FoldedConv(self.feat_proj)

    def forward(self, features, depth):
        if _needs_autograd(self, features, depth):
            return self.feat_proj(features).unsqueeze(2) * depth.unsqueeze(1)
        feat = self._f.run(_to_nhwc(features, ops.DT_F32), ops.DT_F32, relu=False)  # (BN,H,W,C) fp32
        return feat.permute(0, 3, 1, 2).unsqueeze(2) * depth.unsqueeze(1)


class BEVEncoderTransformer(nn.Module):
    """1x1 compress conv-BN-ReLU -> deformable-attention transformer layer -> 3x3/3x3/1x1 seg head.
    Training under bf16 autocast on the GPU: the convs run on the HIP units too (`_train_native_ok`; the 1x1 unit,
    two `_ConvBNActFn` units with the conv bias absorbed by the train-mode BatchNorm, the 64-channel head kernels);
    LSS_BEV_ENCODER_NATIVE=0 and every other case take the torch composition."""

    def __init__(self, in_channels, out_channels=4, precision=None):
        super().__init__()
        self.compress = nn.Sequential(nn.Conv2d(in_channels, 256, 1), nn.BatchNorm2d(256), nn.ReLU(inplace=True))
        self.transformer = LightweightBEVTransformer(d_model=256, n_heads=8, dim_feedforward=1024, dropout=0.1,
                                                     precision=precision)
        self.seg_head = nn.Sequential(
            nn.Conv2d(256, 128, 3, padding=1), nn.BatchNorm2d(128), nn.ReLU(inplace=True),
            nn.Conv2d(128, 64, 3, padding=1), nn.BatchNorm2d(64), nn.ReLU(inplace=True),
            nn.Conv2d(64, out_channels, 1))
        self.precision = precision
        self._fc = _FoldedConv(self.compress[0], self.compress[1])
        self._fs0 = _FoldedConv(self.seg_head[0], self.seg_head[1])
        self._fs1 = _FoldedConv(self.seg_head[3], self.seg_head[4])
        self._fs2 = _FoldedConv(self.seg_head[6])

    def forward_nhwc(self, x, dt):
        """HIP path.  x (B,H,W,C_in) NHWC in dt -> seg (B,out_C,H,W) fp32 NCHW, refined (B,H,W,256) NHWC in dt."""
        h = self._fc.run(x, dt, relu=True)
        refined = self.transformer.forward_nhwc(h, dt)
        s = self._fs0.run(refined, dt, relu=True)
        head = self.seg_head[6]
        if dt == ops.DT_BF16 and self.seg_head[3].out_channels == 64 and head.out_channels <= 64:
            # second 3x3 + BN + ReLU + the 1x1 classifier in ONE launch, NCHW fp32 out: the 64-channel
            # activation is never stored (ref: model_vovnet_transformer.py:139-143)
            w1, sc1, sh1 = self._fs1.get(dt)
            hw = head.weight.detach().float().reshape(head.out_channels, -1).contiguous()
            return ops.conv3x3_head_nchw(s, w1, sc1, sh1, hw, head.bias.detach().float().contiguous(), up=1), refined
        s = self._fs1.run(s, dt, relu=True)
        w, _, shift = self._fs2.get(dt)
        seg = ops.conv2d_nhwc(s, w, (1, 1), 1, 0, None, shift, None, False, dt=dt, out_f32=True)
        return seg.permute(0, 3, 1, 2).contiguous(), refined

    def _train_native_ok(self, x):
        """Does this differentiable call take the native route?  (The switch LSS_BEV_ENCODER_NATIVE, a GPU input under
        bf16 autocast - `modules._native_training()` -, the reference's widths 256 / 128 / 64 with 4 or 8 classes and
        a compress width the 1x1 unit takes, and the three BatchNorms in training mode.)"""
        if os.environ.get("LSS_BEV_ENCODER_NATIVE", _BEV_ENCODER_NATIVE_DEFAULT) == "0":
            return False
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4):
            return False
        cc, cb = self.compress[0], self.compress[1]
        s0, b0, s1, b1, head = (self.seg_head[i] for i in (0, 1, 3, 4, 6))
        if (cc.out_channels, s0.in_channels, s0.out_channels, s1.in_channels, s1.out_channels) != (256, 256, 128, 128, 64):
            return False
        if (head.in_channels != 64 or head.out_channels not in (4, 8) or head.kernel_size != (1, 1)
                or head.stride != (1, 1) or head.bias is None):
            return False
        return (modules._conv1x1_unit_ok(cc, cb, x)
                and all(modules._biased_conv3x3_unit_ok(c, b, True, c.in_channels) for c, b in ((s0, b0), (s1, b1))))

    def _train_native_features(self, x):
        """compress unit -> transformer (unchanged) -> the two 3x3 units; returns (the 64-channel activation the head
        reads, refined), both logical NCHW views of NHWC memory."""
        h = modules._train_conv1x1_bn_act(self.compress[0], self.compress[1], x)
        refined = self.transformer(h)
        s = modules._train_conv_bn_act(self.seg_head[0], self.seg_head[1], refined, relu=True)
        return modules._train_conv_bn_act(self.seg_head[3], self.seg_head[4], s, relu=True), refined

    def forward(self, x):
        """(B, C_in, H, W) -> seg (B, out_C, H, W), refined (B, 256, H, W)."""
        if _needs_autograd(self, x):
            if self._train_native_ok(x):
                BEV_ENCODER_CALLS["native"] += 1
                s, refined = self._train_native_features(x)
                return head_1x1(s, self.seg_head[6]).float(), refined
            BEV_ENCODER_CALLS["composition"] += 1
            refined = self.transformer(self.compress(x))
            return self.seg_head(refined), refined
        dt = _dt(self.precision)
        seg, refined = self.forward_nhwc(_to_nhwc(x, dt), dt)
        return seg, ops.nhwc_to_nchw(refined, dt)

    def forward_loss(self, x, target, class_weight):
        """(nn.CrossEntropyLoss(weight=class_weight)(seg, target), refined) for `seg, refined = self(x)`: the BEV term
        of MultiTaskLoss (ref train_vovnet_transformer.py:83-84, 107), the counterpart of `LSS.forward_loss`.  On the
        native route the classifier and the loss are one kernel per direction and the logits never reach HBM."""
        if _needs_autograd(self, x) and self._train_native_ok(x):
            BEV_ENCODER_CALLS["native"] += 1
            s, refined = self._train_native_features(x)
            return head_weighted_cross_entropy(s, self.seg_head[6], target, class_weight), refined
        seg, refined = self(x)
        return weighted_cross_entropy(seg.float(), target, class_weight), refined


# ----------------------------------------------------------------------------
# TXT branch.  The modules below are stock PyTorch and define the state_dict; at inference the pyramid and the ASPP
# (about a seventh of the step's FLOPs) run on K13 through `_CameraBranchPlan`, the six-token tail stays on library ops.
# ----------------------------------------------------------------------------
class AdaptiveFeaturePyramid(nn.Module):
    """Two dilated 3x3 branches (d=1, d=2) fused by a 1x1 conv."""

    def __init__(self, in_channels=768, out_channels=256):
        super().__init__()

        def branch(d):
            return nn.Sequential(nn.Conv2d(in_channels, out_channels, 3, padding=d, dilation=d),
                                 nn.BatchNorm2d(out_channels), nn.ReLU(inplace=True))

        self.scale1 = branch(1)
        self.scale2 = branch(2)
        self.fusion = nn.Sequential(nn.Conv2d(out_channels * 2, out_channels, 1), nn.BatchNorm2d(out_channels),
                                    nn.ReLU(inplace=True))

    def forward(self, x):
        return self.fusion(torch.cat([self.scale1(x), self.scale2(x)], dim=1))


class _CameraBranchPlan:
    """The folded operands of c3 -> scene tokens for K13: one `_FoldedConv` per conv of `feature_pyramid` and
    `sceneunder` (packed bf16 weights, BatchNorm folded to (scale, shift); rebuilt when a source tensor changes)."""

    MID = 256

    def __init__(self, pyramid, sceneunder):
        aspp = sceneunder[0]
        self.modules = self.convs_of(pyramid, sceneunder)
        self.pyr = [_FoldedConv(b[0], b[1]) for b in (pyramid.scale1, pyramid.scale2)]
        self.fusion = _FoldedConv(pyramid.fusion[0], pyramid.fusion[1])
        self.aspp = [_FoldedConv(c[0], c[1]) for c in list(aspp.convs)[:4]]
        self.pool = _FoldedConv(aspp.convs[4][1], aspp.convs[4][2], pack=False)
        self.project = _FoldedConv(aspp.project[0], aspp.project[1], pack=False)

    @staticmethod
    def convs_of(pyramid, sceneunder):
        """The conv / BN modules the plan reads, or None when the two modules do not have the reference's structure
        (256 mid channels, two dilated pyramid branches, an ASPP with three atrous rates of any value)."""
        M = _CameraBranchPlan.MID
        try:
            aspp = sceneunder[0]
            s1, s2, fu = pyramid.scale1, pyramid.scale2, pyramid.fusion
            convs, proj = list(aspp.convs), aspp.project
            if len(sceneunder) != 1 or len(convs) != 5 or not isinstance(convs[4][0], nn.AdaptiveAvgPool2d):
                return None
            cin = s1[0].in_channels
            ok = (_conv_is(s1[0], 3, cin, M, True) and _conv_is(s2[0], 3, cin, M, True) and _conv_is(fu[0], 1, 2 * M, M, True)
                  and _conv_is(convs[0][0], 1, M, M, False) and all(_conv_is(c[0], 3, M, M, False) for c in convs[1:4])
                  and _conv_is(convs[4][1], 1, M, M, False) and _conv_is(proj[0], 1, 5 * M, M, False)
                  and convs[4][0].output_size in (1, (1, 1)))
            pairs = [(s1[0], s1[1]), (s2[0], s2[1]), (fu[0], fu[1])] + [(c[0], c[1]) for c in convs[:4]] + \
                    [(convs[4][1], convs[4][2]), (proj[0], proj[1])]
            relus = [s1[2], s2[2], fu[2]] + [c[2] for c in convs[:4]] + [convs[4][3], proj[2]]
            if not ok or not all(_bn_is(bn, M) for _, bn in pairs) or not all(isinstance(r, nn.ReLU) for r in relus):
                return None
            return [m for pair in pairs for m in pair]
        except (AttributeError, IndexError, TypeError):
            return None

    def current(self, pyramid, sceneunder):
        mods = self.convs_of(pyramid, sceneunder)
        return mods is not None and len(mods) == len(self.modules) and all(a is b for a, b in zip(mods, self.modules))

    def tokens(self, c3):
        """(BN, Cin, H, W) fp32 -> (BN, 256) fp32 in six launches; no map wider than the 1024-channel ASPP buffer."""
        dt = ops.DT_BF16
        M = self.MID
        x = _to_nhwc(c3, dt)                                                         # L0
        BN, H, W, _ = x.shape
        dev = x.device
        pyr = torch.empty(BN, H, W, 2 * M, dtype=torch.bfloat16, device=dev)
        branches = []
        for i, f in enumerate(self.pyr):
            w, sc, sh = f.get(dt)
            branches.append((w, 3, f.conv.dilation[0], sc, sh, i * M))
        ops.tapconv(x, branches, y=pyr)                                              # L1: both pyramid branches
        w, sc, sh = self.fusion.get(dt)
        p = torch.empty(BN, H, W, M, dtype=torch.bfloat16, device=dev)
        p_mean = ops.tapconv(pyr, [(w, 1, 1, sc, sh, 0)], y=p, means=True)           # L2: fusion 1x1 + mean of p
        cat = torch.empty(BN, H, W, 4 * M, dtype=torch.bfloat16, device=dev)
        branches = []
        for i, f in enumerate(self.aspp):
            w, sc, sh = f.get(dt)
            branches.append((w, f.conv.kernel_size[0], f.conv.dilation[0], sc, sh, i * M))
        ops.tapconv(p, branches, y=cat)                                              # L3: the four conv branches
        _, gsc, gsh = self.pool.get(dt)
        _, jsc, jsh = self.project.get(dt)
        wg = self.pool.image("f32", lambda w32: w32[:, :, 0, 0].contiguous())
        wj = self.project.image("main", lambda w32: ops.pack_conv_weight(w32[:, :4 * M].contiguous(), dt))
        wjp = self.project.image("pool", lambda w32: w32[:, 4 * M:, 0, 0].contiguous())
        bias = ops.camera_pool_bias(p_mean, wg, gsc, gsh, wjp)                       # L3': pooled branch -> bias
        return ops.tapconv(cat, [(wj, 1, 1, jsc, jsh, 0)], img_bias=bias, means=True)  # L4: project + mean


def _mha_is(m):
    return (type(m) is nn.MultiheadAttention and m.embed_dim == 256 and m.num_heads == 4 and m.batch_first
            and m._qkv_same_embed_dim and m.in_proj_bias is not None and m.out_proj.bias is not None
            and m.bias_k is None and m.bias_v is None and not m.add_zero_attn)


def _linear_is(m, cin, cout):
    return (type(m) is nn.Linear and m.in_features == cin and m.bias is not None
            and (cout is None or m.out_features == cout))


def _ln_is(m, c):
    return (type(m) is nn.LayerNorm and tuple(m.normalized_shape) == (c,) and m.elementwise_affine
            and m.bias is not None)


def _gelu_is(m):
    return type(m) is nn.GELU and m.approximate == "none"


class _CameraTailPlan:
    """What K14 reads of camera_transformer, bev_fusion and unified_predictor: the modules whose structure, mode and
    hooks decide the route, and the parameter tensors, handed to the kernel where they lie (no copies: an in-place edit,
    a `load_state_dict` or a `.to()` is seen by the next call)."""

    def __init__(self, model):
        self.modules = self.modules_of(model)
        self._ids_ok = None  # (camera_ids' storage and version) that was found equal to arange

    @staticmethod
    def modules_of(model):
        """Every module the tail runs (the three and their submodules), or None when they do not have the reference's
        structure: d_model 256, 4 heads, batch_first, one in_proj, biases, no bias_k / add_zero_attn; FFN 256 -> 512 ->
        256 and predictor 256 -> 512 -> 256 with erf GELUs and affine LayerNorms."""
        try:
            ct, bf, up = model.camera_transformer, model.bev_fusion, model.unified_predictor
            if type(up) is not UnifiedPredictor:
                return None
            enc = up.encoder
            if not (len(enc) == 7 and _linear_is(enc[0], 256, 512) and _ln_is(enc[1], 512) and _gelu_is(enc[2])
                    and type(enc[3]) is nn.Dropout and _linear_is(enc[4], 512, 256) and _ln_is(enc[5], 256)
                    and _gelu_is(enc[6]) and enc[1].eps == enc[5].eps and _linear_is(up.action_head, 256, None)
                    and _linear_is(up.desc_head, 256, None) and up.camera_weights.dim() == 1):
                return None
            if ct is not None:
                f = ct.ffn
                if not (type(ct) is LightweightCameraTransformer and _mha_is(ct.self_attn)
                        and type(ct.cam_embed) is nn.Embedding and ct.cam_embed.embedding_dim == 256
                        and ct.cam_embed.max_norm is None and _ln_is(ct.norm1, 256) and _ln_is(ct.norm2, 256)
                        and ct.norm1.eps == ct.norm2.eps and len(f) == 4 and _linear_is(f[0], 256, 512)
                        and _gelu_is(f[1]) and type(f[2]) is nn.Dropout and _linear_is(f[3], 512, 256)):
                    return None
            if bf is not None and not (type(bf) is BEVCameraFusion and _mha_is(bf.cross_attn) and _ln_is(bf.norm, 256)):
                return None
            return [m for top in (ct, bf, up) if top is not None for m in top.modules()]
        except (AttributeError, TypeError, IndexError):
            return None

    def current(self, model):
        mods = self.modules_of(model)
        return mods is not None and len(mods) == len(self.modules) and all(a is b for a, b in zip(mods, self.modules))

    def quiet(self):
        """Eval mode everywhere and no forward (pre-)hook, on these modules or globally: a hook must keep seeing real
        module calls."""
        from torch.nn.modules import module as _m
        if _m._global_forward_hooks or _m._global_forward_pre_hooks:
            return False
        return not any(m.training or m._forward_hooks or m._forward_pre_hooks for m in self.modules)

    def ids_are_arange(self, ids, n):
        """camera_ids == arange(n): compared once per buffer version (a device read), never per step."""
        if ids.dim() != 1 or ids.numel() != n or ids.dtype != torch.long:
            return False
        key = (ids.data_ptr(), ids._version, ids.device)
        if self._ids_ok != key:
            if not torch.equal(ids.detach().cpu(), torch.arange(n)):
                return False
            self._ids_ok = key
        return True

    @staticmethod
    def params(model):
        """{field of lss_camera_tail_desc_t: the modules' own tensor}."""
        ct, bf, up = model.camera_transformer, model.bev_fusion, model.unified_predictor
        enc = up.encoder
        p = {"cam_w": up.camera_weights, "enc1_w": enc[0].weight, "enc1_b": enc[0].bias, "ln1_w": enc[1].weight,
             "ln1_b": enc[1].bias, "enc2_w": enc[4].weight, "enc2_b": enc[4].bias, "ln2_w": enc[5].weight,
             "ln2_b": enc[5].bias, "act_w": up.action_head.weight, "act_b": up.action_head.bias,
             "desc_w": up.desc_head.weight, "desc_b": up.desc_head.bias}
        eps = {"eps_pred": enc[1].eps}
        if ct is not None:
            sa, f = ct.self_attn, ct.ffn
            p.update(cam_embed=ct.cam_embed.weight, sa_in_w=sa.in_proj_weight, sa_in_b=sa.in_proj_bias,
                     sa_out_w=sa.out_proj.weight, sa_out_b=sa.out_proj.bias, norm1_w=ct.norm1.weight,
                     norm1_b=ct.norm1.bias, ffn1_w=f[0].weight, ffn1_b=f[0].bias, ffn2_w=f[3].weight, ffn2_b=f[3].bias,
                     norm2_w=ct.norm2.weight, norm2_b=ct.norm2.bias)
            eps["eps_cam"] = ct.norm1.eps
        if bf is not None:
            ca = bf.cross_attn
            p.update(ca_in_w=ca.in_proj_weight, ca_in_b=ca.in_proj_bias, ca_out_w=ca.out_proj.weight,
                     ca_out_b=ca.out_proj.bias, norm3_w=bf.norm.weight, norm3_b=bf.norm.bias)
            eps["eps_fuse"] = bf.norm.eps
        return p, eps


class LightweightCameraTransformer(nn.Module):
    """One post-norm transformer layer over the N camera tokens of a sample."""

    def __init__(self, d_model=256, n_heads=4, dropout=0.1, n_cameras=6):
        super().__init__()
        self.cam_embed = nn.Embedding(n_cameras, d_model)
        self.self_attn = nn.MultiheadAttention(embed_dim=d_model, num_heads=n_heads, dropout=dropout, batch_first=True)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.ffn = nn.Sequential(nn.Linear(d_model, d_model * 2), nn.GELU(), nn.Dropout(dropout),
                                 nn.Linear(d_model * 2, d_model))

    def forward(self, x, camera_ids):
        x = x + self.cam_embed(camera_ids)
        x = self.norm1(x + self.self_attn(x, x, x)[0])
        return self.norm2(x + self.ffn(x))


class BEVCameraFusion(nn.Module):
    """Camera tokens attend to the globally pooled BEV token."""

    def __init__(self, camera_dim=256, bev_dim=256, n_heads=4):
        super().__init__()
        self.cross_attn = nn.MultiheadAttention(embed_dim=camera_dim, num_heads=n_heads, dropout=0.1, batch_first=True)
        self.norm = nn.LayerNorm(camera_dim)

    def forward(self, camera_feat, bev_feat):
        """bev_feat: (B, C, H, W) map, or its global average (B, C) if the caller already pooled it."""
        tok = (bev_feat.mean(dim=(2, 3)) if bev_feat.dim() == 4 else bev_feat).unsqueeze(1)
        return self.norm(camera_feat + self.cross_attn(camera_feat, tok, tok)[0])


class UnifiedPredictor(nn.Module):
    """Softmax-weighted mean over cameras -> shared MLP -> action / description logits."""

    def __init__(self, input_dim=256, num_action_classes=4, num_desc_classes=8, n_cameras=6):
        super().__init__()
        self.camera_weights = nn.Parameter(torch.ones(n_cameras) / n_cameras)
        self.encoder = nn.Sequential(nn.Linear(input_dim, 512), nn.LayerNorm(512), nn.GELU(), nn.Dropout(0.1),
                                     nn.Linear(512, 256), nn.LayerNorm(256), nn.GELU())
        self.action_head = nn.Linear(256, num_action_classes)
        self.desc_head = nn.Linear(256, num_desc_classes)

    def forward(self, camera_features):
        w = F.softmax(self.camera_weights, dim=0).view(1, -1, 1)
        z = self.encoder((camera_features * w).sum(dim=1))
        return self.action_head(z), self.desc_head(z)


class TrunkC3C4(nn.Module):
    """Stand-in for the reference's `VoVNetV2` slot: accepts {'c3','c4'} (or a
    (c3, c4) pair) of trunk feature maps and hands them on."""
    c3_channels = 768
    c4_channels = 1024

    def forward(self, x):
        if isinstance(x, dict):
            return x
        if isinstance(x, (tuple, list)) and len(x) == 2:
            return {"c3": x[0], "c4": x[1]}
        raise RuntimeError(
            "got camera images: the VoVNet trunk of the reference (timm ese_vovnet, third-party weights) is "
            "not bundled; pass backbone=<your trunk module> or feed {'c3': ..., 'c4': ...} feature maps")


class VoVNetBEVTransformer(_LiftSplatMixin, nn.Module):
    def __init__(self, bsize, grid_conf, data_aug_conf, outC=4, vovnet_type="vovnet57", pretrained=True,
                 lss_version="v2", use_camera_attn=True, use_cross_attn=True, backbone=None, precision=None):
        nn.Module.__init__(self)
        self.vovnet_type = vovnet_type
        self.lss_version = lss_version.lower()
        self.use_camera_attn = use_camera_attn
        self.use_cross_attn = use_cross_attn
        if self.lss_version not in {"v1", "v2"}:
            raise ValueError(f"Unsupported lss_version: {lss_version}. Use 'v1' or 'v2'.")
        self._init_grid(bsize, grid_conf, data_aug_conf)
        self.D = 41
        self.C = 128
        self.precision = precision
        self.backbone = backbone if backbone is not None else TrunkC3C4()
        c3c, c4c = self.backbone.c3_channels, self.backbone.c4_channels
        if self.lss_version == "v2":
            self.depth_net = MultiScaleDepthNet(c3_channels=c3c, c4_channels=c4c, depth_channels=self.D,
                                                precision=precision)
        else:
            self.depth_net = StandardDepthNet(c3_channels=c3c, depth_channels=self.D, precision=precision)
        self.cam_encode = CamEncodeV2(D=self.D, C_in=c3c, C_out=self.C)
        self.bev_encoder = BEVEncoderTransformer(in_channels=self.C * int(self.nx[2].item()), out_channels=outC,
                                                 precision=precision)
        self.feature_pyramid = AdaptiveFeaturePyramid(in_channels=c3c, out_channels=256)
        self.sceneunder = SceneUnder(in_channels=256)
        self.camera_names = data_aug_conf["cams"]
        self.n_cameras = len(self.camera_names)
        self.register_buffer("camera_ids", torch.arange(self.n_cameras, dtype=torch.long))
        self.camera_transformer = LightweightCameraTransformer(256, 4, 0.1, self.n_cameras) if use_camera_attn else None
        self.bev_fusion = BEVCameraFusion(256, 256, 4) if use_cross_attn else None
        self.unified_predictor = UnifiedPredictor(256, 4, 8, self.n_cameras)

    # get_geometry / voxel_pooling / create_frustum: _LiftSplatMixin (same arithmetic as
    # ref :483-554, which repeats src/model_BEV_TXT.py:37-126)

    def get_voxels(self, c3, c4, rots, trans, intrins, post_rots, post_trans, layout=ops.BEV_NCHW_F32):
        """Trunk maps + calibration -> BEV grid (B, C*nz, nx, ny) [logical shape]."""
        BN, _, fH, fW = c3.shape
        B = rots.shape[0]  # (a data.CalibrationPack has .shape = (B, N) too)
        Ncam = BN // B
        cshape = tuple(rots.shape[:2]) if trans is None else tuple(trans.shape[:2])
        if BN % B != 0 or cshape != (B, Ncam):
            raise RuntimeError("features for %d images do not match %s calibrations" % (BN, cshape))
        if (self.D, fH, fW) != tuple(self.frustum.shape[:3]):
            raise RuntimeError("feature map %dx%d / D=%d does not match the frustum %s"
                               % (fH, fW, self.D, tuple(self.frustum.shape[:3])))
        if _needs_autograd(self.depth_net, c3, c4) or _needs_autograd(self.cam_encode, c3):
            if self._lift_native_ok(c3, c4):
                return _native_lift(self, c3, c4, (rots, trans, intrins, post_rots, post_trans), B, Ncam, layout)
            # the torch composition: library ops for the heads, then the differentiable voxel pooling on the
            # materialised lifted tensor (CPU tensors, shapes the kernels refuse, LSS_VOVNET_LIFT_NATIVE=0)
            LIFT_CALLS["composition"] += 1
            depth = self.depth_net(c3, c4)
            cam = self.cam_encode(c3, depth).view(B, Ncam, self.C, self.D, fH, fW).permute(0, 1, 3, 4, 5, 2)
            return self.voxel_pooling(self.get_geometry(rots, trans, intrins, post_rots, post_trans), cam)
        with ops.region("lift_splat_level"):
            # depth heads + CamEncodeV2 (K2v), then geometry + bucketing + splat behind one native call: the
            # region-bucketed pipeline at C = 128 (LDS region histograms, fixed-point region splat)
            dev = self.frustum.device
            nx = self._nx_ints()
            inv_pr, comb, ptr, trn = self._device_calib(dev, rots, trans, intrins, post_rots, post_trans)
            ws = self._workspace(B * Ncam * self.D * fH * fW, B * nx[0] * nx[1] * nx[2], dev)
            depth, feat = self.depth_net.depth_and_context(c3, c4, self.cam_encode)
            with _histogram_guard(ws):  # a failed call must not leave the zero-between-calls words dirty
                return ops.lift_splat_from_heads(self.frustum.detach(), inv_pr, ptr, comb, trn, self.dx.detach(),
                                                 self.bx.detach(), depth, feat, ws, (B, Ncam, self.D, fH, fW, self.C),
                                                 nx, layout)

    def _lift_native_ok(self, c3, c4):
        """May a differentiable `get_voxels` take the native nodes?  GPU tensors, constant grid, and shapes K2v, K7,
        K10 and the splat accept; LSS_VOVNET_LIFT_NATIVE=0 keeps the torch composition."""
        if os.environ.get("LSS_VOVNET_LIFT_NATIVE", "1") == "0":
            return False
        v2 = self.lss_version == "v2"
        if not (c3.is_cuda and self.frustum.is_cuda and (c4.is_cuda if v2 else True)):
            return False
        if self.frustum.requires_grad or self.dx.requires_grad or self.bx.requires_grad:
            return False
        # the nodes compute in fp32: fp32 modules, and fp32 maps unless autocast casts them at the nodes' door
        params = list(self.depth_net.parameters()) + list(self.cam_encode.parameters()) + [self.frustum]
        if any(p.dtype != torch.float32 for p in params):
            return False
        maps = [c3] + ([c4] if v2 else [])
        if any(t.dtype != torch.float32 for t in maps) and not torch.is_autocast_enabled("cuda"):
            return False
        BN, Cf, fH, fW = c3.shape
        heads = [self.depth_net.depth_c3, self.depth_net.depth_c4] if v2 else [self.depth_net.depth_head]
        Cd = heads[0][3].in_channels
        if any(h[3].in_channels != Cd or h[3].out_channels != self.D for h in heads) or self.D > 64:
            return False
        if Cd % 64 or Cf % 64 or self.C not in (64, 128) or self.cam_encode.feat_proj.in_channels != Cf:
            return False
        hws = [fH * fW] + ([c4.shape[2] * c4.shape[3]] if v2 else [])
        return (all(ops.pointwise_conv_bwd_ok(BN, Cd, self.D, hw) for hw in hws)
                and ops.pointwise_conv_bwd_ok(BN, Cf, self.C, fH * fW))

    def _camera_branch_native_ok(self, c3):
        """Does `scene_tokens` take K13?  Eval without autograd, a GPU fp32 map, bf16 precision, the reference's module
        structure, a shape `lss_tapconv_ok` accepts; LSS_CAMERA_BRANCH_NATIVE=0 keeps the library composition."""
        if os.environ.get("LSS_CAMERA_BRANCH_NATIVE", _CAMERA_BRANCH_NATIVE_DEFAULT) == "0":
            return False
        if not (torch.is_tensor(c3) and c3.is_cuda and c3.dim() == 4 and c3.dtype == torch.float32):
            return False
        if _dt(self.precision) != ops.DT_BF16:
            return False
        fp, su = self.feature_pyramid, self.sceneunder
        if fp.training or su.training or _needs_autograd(fp, c3) or _needs_autograd(su):
            return False
        plan = self.__dict__.get("_camera_plan")
        if plan is None or not plan.current(fp, su):
            if _CameraBranchPlan.convs_of(fp, su) is None:
                return False
            plan = self.__dict__["_camera_plan"] = _CameraBranchPlan(fp, su)
        if any(m.weight.device != c3.device or m.weight.dtype != torch.float32 for m in plan.modules):
            return False
        BN, Cin, H, W = c3.shape
        return Cin == plan.pyr[0].conv.in_channels and all(
            ops.tapconv_ok(BN, H, W, ci, _CameraBranchPlan.MID) for ci in (Cin, 256, 512, 1024))

    def _camera_branch_train_call(self, c3):
        """Is this `scene_tokens` call a training call: a module in training mode, or gradients wanted?"""
        fp, su = self.feature_pyramid, self.sceneunder
        if fp.training or su.training:
            return True
        return torch.is_grad_enabled() and ((torch.is_tensor(c3) and c3.requires_grad) or any(
            p.requires_grad for m in (fp, su) for p in m.parameters()))

    def _camera_branch_train_native_ok(self, c3):
        """Does a differentiable `scene_tokens` take the native conv-BN units?  Autograd needed, bf16 autocast, a GPU
        map, `feature_pyramid` and `sceneunder` in training mode with the reference's structure and no forward or
        backward hooks on them or their children (here and globally), and every unit's own guard;
        LSS_CAMERA_BRANCH_TRAIN_NATIVE=0 keeps the library composition."""
        if os.environ.get("LSS_CAMERA_BRANCH_TRAIN_NATIVE", _CAMERA_BRANCH_TRAIN_NATIVE_DEFAULT) == "0":
            return False
        if not (torch.is_tensor(c3) and c3.is_cuda and c3.dim() == 4 and c3.dtype in (torch.float32, torch.bfloat16)):
            return False
        fp, su = self.feature_pyramid, self.sceneunder
        if not (fp.training and su.training and modules._native_training()):
            return False
        if not (_needs_autograd(fp, c3) or _needs_autograd(su)):
            return False
        mods = _CameraBranchPlan.convs_of(fp, su)
        if mods is None:
            return False
        from torch.nn.modules import module as _m
        if (_m._global_forward_hooks or _m._global_forward_pre_hooks or _m._global_backward_hooks
                or _m._global_backward_pre_hooks):
            return False
        children = [c for top in (fp, su) for c in top.modules()]
        if any(not c.training or c._forward_hooks or c._forward_pre_hooks or c._backward_hooks or c._backward_pre_hooks
               for c in children):
            return False
        if any(m.weight.device != c3.device for m in mods):
            return False
        BN, Cin, H, W = c3.shape
        M = _CameraBranchPlan.MID
        aspp = su[0]
        x, pyr, p, cat = (_MapLike(BN, c, H, W) for c in (Cin, 2 * M, M, 4 * M))
        s1, s2, fu, convs, proj = fp.scale1, fp.scale2, fp.fusion, aspp.convs, aspp.project
        pool_bn = convs[4][2]
        return (modules._biased_conv3x3_unit_ok(s1[0], s1[1], True, Cin) and "_lss_sync" not in s1[1].__dict__
                and s1[0].weight.dtype == torch.float32
                and modules._tapconv_unit_ok(s2[0], s2[1], x)
                and modules._conv1x1_unit_ok(fu[0], fu[1], pyr)
                and modules._conv1x1_unit_ok(convs[0][0], convs[0][1], p)
                and all(modules._tapconv_unit_ok(c[0], c[1], p) for c in convs[1:4])
                and modules._tapconv_unit_ok(proj[0], proj[1], cat, cin=4 * M)
                and "_lss_sync" not in pool_bn.__dict__ and convs[4][1].weight.dtype == torch.float32)

    def _camera_branch_train_tokens(self, c3):
        """The training form of `scene_tokens` on the native conv-BN units (the caller has checked
        `_camera_branch_train_native_ok`): no library convolution in either direction.  c3 becomes bf16 NHWC once;
        the d = 1 pyramid branch is the fused 3x3 unit, the d = 2 branch and the three atrous convs are tap-list
        units, the fusion and the ASPP's 1x1 branch are 1x1 units.  The pooled branch is constant over the image:
        it runs in fp32 on (BN, 256) rows through the modules' own parameters and BatchNorm and enters the
        projection as a per-image bias, so the projection reads the 1024-channel concat of the conv branches only."""
        fp, aspp = self.feature_pyramid, self.sceneunder[0]
        M = _CameraBranchPlan.MID
        BN = c3.shape[0]

        def cat(maps):  # logical NCHW views of NHWC memory -> one NHWC buffer, again as a logical NCHW view
            return torch.cat([t.permute(0, 2, 3, 1) for t in maps], dim=3).permute(0, 3, 1, 2)

        x = modules._nhwc_bf16(c3).permute(0, 3, 1, 2)
        s1 = modules._train_conv_bn_act(fp.scale1[0], fp.scale1[1], x, True)
        s2 = modules._train_tapconv_bn_act(fp.scale2[0], fp.scale2[1], x)
        p = modules._train_conv1x1_bn_act(fp.fusion[0], fp.fusion[1], cat([s1, s2]))
        convs, proj = aspp.convs, aspp.project
        branches = [modules._train_conv1x1_bn_act(convs[0][0], convs[0][1], p)]
        branches += [modules._train_tapconv_bn_act(c[0], c[1], p) for c in convs[1:4]]
        wj = proj[0].weight
        with torch.autocast("cuda", enabled=False):
            g = p.mean(dim=(2, 3), dtype=torch.float32)
            g = F.linear(g, convs[4][1].weight.view(M, M))
            g = F.relu(convs[4][2](g.view(BN, M, 1, 1))).view(BN, M)
            img_bias = F.linear(g, wj[:, 4 * M:, 0, 0])
        y = modules._train_tapconv_bn_act(proj[0], proj[1], cat(branches), weight=wj[:, :4 * M], img_bias=img_bias)
        return proj[3](y).mean(dim=(2, 3), dtype=torch.float32)

    def scene_tokens(self, c3):
        """c3 (B*N, C, fH, fW) -> the per-camera scene tokens (B*N, 256) fp32: feature pyramid, ASPP, mean over the map
        (ref :612-620).  At inference in bf16 on the GPU this is K13 (six launches, the scene map is never written);
        a training call under bf16 autocast on the GPU runs on the native conv-BN units (`_camera_branch_train_tokens`);
        every other call - fp32 precision, CPU, fp16 autocast, foreign modules - is the library composition."""
        if self._camera_branch_native_ok(c3):
            CAMERA_BRANCH_CALLS["native"] += 1
            with ops.region("camera_branch"):
                return self._camera_plan.tokens(c3)
        if self._camera_branch_train_call(c3):
            if self._camera_branch_train_native_ok(c3):
                CAMERA_BRANCH_TRAIN_CALLS["native"] += 1
                with ops.region("camera_branch_train"):
                    return self._camera_branch_train_tokens(c3)
            CAMERA_BRANCH_TRAIN_CALLS["composition"] += 1
        CAMERA_BRANCH_CALLS["composition"] += 1
        scene = self.sceneunder(self.feature_pyramid(c3))
        return scene.mean(dim=(2, 3))

    def _camera_tail_native_ok(self, tokens, refined):
        """Does the inference branch of `forward` take K14 behind the scene tokens?  No autograd, every tail module in
        eval mode and free of forward hooks (here and globally), the reference's structure, fp32 parameters on the
        tokens' GPU, shapes `lss_camera_tail_ok` accepts; LSS_CAMERA_TAIL_NATIVE=0 keeps the library composition.
        Returns the kernel's operands, or None."""
        if os.environ.get("LSS_CAMERA_TAIL_NATIVE", _CAMERA_TAIL_NATIVE_DEFAULT) == "0":
            return None
        if not (torch.is_tensor(tokens) and tokens.is_cuda and tokens.dim() == 3 and tokens.dtype == torch.float32
                and tokens.shape[2] == 256):
            return None
        ct, bf, up = self.camera_transformer, self.bev_fusion, self.unified_predictor
        tops = [m for m in (ct, bf, up) if m is not None]
        if any(m.training for m in tops) or _needs_autograd(tops[0], tokens, refined) or any(
                _needs_autograd(m) for m in tops[1:]):
            return None
        plan = self.__dict__.get("_tail_plan")
        if plan is None or not plan.current(self):
            if _CameraTailPlan.modules_of(self) is None:
                return None
            plan = self.__dict__["_tail_plan"] = _CameraTailPlan(self)
        if not plan.quiet():
            return None
        B, N = tokens.shape[:2]
        if up.camera_weights.numel() != N:
            return None
        if ct is not None and not (ct.cam_embed.num_embeddings >= N and plan.ids_are_arange(self.camera_ids, N)):
            return None
        if bf is not None and not (torch.is_tensor(refined) and refined.device == tokens.device and refined.dim() == 4
                                   and refined.shape[0] == B and refined.shape[3] == 256 and refined.is_contiguous()
                                   and refined.dtype in (torch.bfloat16, torch.float32)):
            return None
        params, eps = plan.params(self)
        for k, t in params.items():
            if t.dtype != torch.float32 or t.device != tokens.device or not t.is_contiguous():
                return None
            if t.dim() == 2 and t.data_ptr() % 16:  # the kernel reads matrix rows 16 bytes at a time
                return None
        if not ops.camera_tail_ok(B, N, up.action_head.out_features, up.desc_head.out_features):
            return None
        params.update(eps)
        return params

    def forward(self, imgs, rots, trans, intrins, post_rots, post_trans):
        """imgs: (B*N,3,H,W) / (B,N,3,H,W) camera images for a real trunk, or the
        trunk's {'c3','c4'} maps for the default pass-through.  Returns
        (bev_seg (B,outC,X,Y), action (B,4), description (B,8))."""
        if torch.is_tensor(imgs) and imgs.dim() == 5:
            imgs = imgs.reshape(-1, *imgs.shape[2:])
        B = rots.shape[0]
        feats = self.backbone(imgs)
        c3, c4 = feats["c3"], feats["c4"]
        N = c3.shape[0] // B

        be = self.bev_encoder
        if _needs_autograd(be, c3, c4) or _needs_autograd(self.depth_net) or _needs_autograd(self.cam_encode):
            bev_seg, bev_refined = be(self.get_voxels(c3, c4, rots, trans, intrins, post_rots, post_trans))
            bev_pooled = bev_refined.mean(dim=(2, 3))
        else:  # the BEV grid goes to the encoder channels-last in the conv dtype: no NCHW fp32 round trip
            dt = _dt(be.precision)
            layout = ops.BEV_NHWC_BF16 if dt == ops.DT_BF16 else ops.BEV_NHWC_F32
            grid = self.get_voxels(c3, c4, rots, trans, intrins, post_rots, post_trans, layout)
            bev_seg, refined = be.forward_nhwc(grid.permute(0, 2, 3, 1), dt)
            return (bev_seg,) + self.scene_outputs(self.scene_tokens(c3).view(B, N, -1), refined)

        tokens = self.scene_tokens(c3).view(B, N, -1)
        CAMERA_TAIL_CALLS["composition"] += 1
        return (bev_seg,) + self._tail(tokens, bev_pooled)

    def scene_outputs(self, tokens, refined):
        """The inference branch behind the scene tokens: tokens (B, N, 256) fp32 and the refined BEV map (B, X, Y, 256),
        channels-last in the conv dtype -> (action, description).  K14 when `_camera_tail_native_ok` (two launches:
        `bev_pool` + `camera_tail`, no fp32 copy of the map), else the pooled map through the three modules."""
        params = self._camera_tail_native_ok(tokens, refined)
        if params is not None:
            CAMERA_TAIL_CALLS["native"] += 1
            with ops.region("six_token_tail"):
                if self.bev_fusion is None:
                    return ops.camera_tail(tokens.contiguous(), params)
                R = refined.shape[1] * refined.shape[2]
                return ops.camera_tail(tokens.contiguous(), params, ops.bev_pool(refined), 1.0 / R)
        CAMERA_TAIL_CALLS["composition"] += 1
        return self._tail(tokens, refined.float().mean(dim=(1, 2)))

    def _tail(self, tokens, bev_pooled):
        B = tokens.shape[0]
        if self.camera_transformer is not None:
            tokens = self.camera_transformer(tokens, self.camera_ids.unsqueeze(0).expand(B, -1))
        if self.bev_fusion is not None:
            tokens = self.bev_fusion(tokens, bev_pooled)
        action, description = self.unified_predictor(tokens)
        return action, description


def _native_lift(model, c3, c4, calib, B, Ncam, layout):
    """The differentiable lift-splat level on the native nodes: torch 3x3 conv-BN-ReLU (+ v2's fusion tail) ->
    `_HeadProjFn` -> `_HeadsLiftSplatFn`."""
    LIFT_CALLS["native"] += 1
    BN, _, fH, fW = c3.shape
    with ops.region("lift_splat_level_train"):
        dev = model.frustum.device
        nx = model._nx_ints()
        dcal = tuple(model._device_calib(dev, *calib))
        ws = model._workspace(BN * model.D * fH * fW, B * nx[0] * nx[1] * nx[2], dev)
        u, feat = model.depth_net.pre_softmax_and_context(c3, c4, model.cam_encode)
        return _HeadsLiftSplatFn.apply(u, feat, dcal, (model.frustum.detach(), model.dx.detach(), model.bx.detach()),
                                       ws, (B, Ncam, model.D, fH, fW, model.C), nx, layout)


def compile_model_vovnet_transformer(bsize, grid_conf, data_aug_conf, outC, vovnet_type="vovnet39", pretrained=True,
                                     lss_version="v2", use_camera_attn=True, use_cross_attn=True, **kw):
    return VoVNetBEVTransformer(bsize, grid_conf, data_aug_conf, outC, vovnet_type=vovnet_type,
                                pretrained=pretrained, lss_version=lss_version, use_camera_attn=use_camera_attn,
                                use_cross_attn=use_cross_attn, **kw)
