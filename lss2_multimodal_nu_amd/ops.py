"""Tensor-level wrappers over the C ABI (include/lss_hip.h).

Each function validates shapes/dtypes on the host (a mis-shaped operand must
never reach a kernel), allocates outputs with torch, and enqueues the kernel on
torch's current HIP stream.  No CPU / eager fallbacks exist here.
"""
import ctypes
import os
import threading

import torch

from . import _native as N
from ._native import (ACT_GELU, ACT_NONE, ACT_RELU, BEV_NCHW_F32, BEV_NHWC_BF16, BEV_NHWC_F32, DT_BF16,  # noqa: F401
                      DT_F32, OUT_F32, OUT_HEAD_MAJOR32, PW_NCHW_F32, PW_NHWC_BF16, PW_NHWC_F32, VALUE_HEAD_MAJOR,
                      VALUE_NHWC, W_KS, W_RING)


def _f32c(t, name, shape=None):
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise ValueError("%s must be a contiguous fp32 GPU tensor (got %s %s contiguous=%s)"
                         % (name, t.dtype, t.device, t.is_contiguous()))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t


_DT = {torch.float32: DT_F32, torch.bfloat16: DT_BF16}


def _cached_ws(cache, key, nbytes, device):
    """The uint8 workspace of `nbytes` bytes that `cache` holds under `key`, allocated at the first call."""
    ws = cache.get(key)
    if ws is None:
        ws = cache[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


class KernelTimer:
    """Optional HIP-event brackets around native launches (bench.py uses it for
    the roofline numbers).  Events are recorded on torch's current stream - the
    stream the kernels are enqueued on."""

    def __init__(self, fine=False, last_conv=False):
        # fine=True brackets every native launch (each bracket costs ~5-10 us of GPU idle
        # time: diagnostics only); fine=False only the regions opened with `region()`.
        # last_conv=True: a recorded conv plan is replayed in two native calls and its LAST launch
        # (BevEncode: up2 3x3 + BN + ReLU + fused 1x1 head, the dominant kernel) gets a bracket of
        # its own, tag "conv_plan_last" - bench.py's separate per-kernel roofline pass.
        self.spans = {}
        self.fine = fine
        self.last_conv = last_conv

    def bracket(self, tag):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.spans.setdefault(tag, []).append((s, e))
        return s, e

    def totals_ms(self):
        """tag -> (launches, total ms); call after a device synchronize."""
        return {t: (len(v), sum(s.elapsed_time(e) for s, e in v)) for t, v in self.spans.items()}


_timer = None


def set_timer(t):
    global _timer
    _timer = t


class _timed:
    def __init__(self, tag, coarse=False):
        self.ev = _timer.bracket(tag) if (_timer is not None and tag and (coarse or _timer.fine)) else None

    def __enter__(self):
        if self.ev:
            self.ev[0].record()

    def __exit__(self, *a):
        if self.ev:
            self.ev[1].record()
        return False


def region(tag):
    """Coarse HIP-event bracket around a group of launches (e.g. all of BevEncode)."""
    return _timed(tag, coarse=True)


# --- hang guards of the loader / consumer kernels (conv_ring.hip, conv_wgrad.hip, chained convs) ---------------------
# Every FULL / FREE flag wait of those kernels is bounded; a wait that hits its bound ends the grid instead of hanging
# the GPU, bumps a device counter and leaves GARBAGE in that launch's output.  The counters are therefore part of the
# product's contract, not a test detail: bench.py reads them after every leg, BevEncode whenever it records a launch
# plan (and every LSS_GUARD_EVERY-th call), dp.GraphedTrainStep in its self-check.
GUARD_COUNTERS = ("lss_conv2d_ring_timeouts", "lss_conv2d_wgrad_timeouts")


def timeout_counters(lib=None):
    """{counter name: value} of the flag-wait timeout counters (0 = every hand-off completed; -1 = the counter could
    not be read).  Synchronises the device (a device-to-host copy of one int each): never call inside a stream capture."""
    L = lib if lib is not None else N.lib()
    return {name[len("lss_conv2d_"):]: int(getattr(L, name)()) for name in GUARD_COUNTERS}


def assert_no_timeouts(where, lib=None):
    """Raise LssNativeError when a loader / consumer hand-off of any launch so far ran into its bound."""
    bad = {k: v for k, v in timeout_counters(lib).items() if v != 0}
    if bad:
        raise N.LssNativeError("%s: flag waits of the loader / consumer kernels hit their bound (%s): the affected "
                               "launches produced garbage" % (where, ", ".join("%s=%d" % kv for kv in sorted(bad.items()))))


def guard_every():
    """LSS_GUARD_EVERY=N: BevEncode checks the counters on every N-th inference call (0 / unset: only when it records a
    launch plan; each check is a device synchronisation)."""
    try:
        return max(0, int(os.environ.get("LSS_GUARD_EVERY", "0")))
    except ValueError:
        return 0


class ConvRecorder:
    """Collects the conv launches of one eager pass (the descriptors `_conv_launch` ran) together with the
    tensors that must outlive them; `ConvPlan` replays the list with ONE native call."""

    def __init__(self):
        self.launches = []  # (kind, N.ConvLaunch)
        self.keep = []

    def add(self, launch, keep):
        self.launches.append((launch.kind, launch))
        self.keep.extend(keep)


_recorder = None


def set_recorder(r):
    global _recorder
    _recorder = r


class ConvPlan:
    def __init__(self, rec, x_in, out):
        n = len(rec.launches)
        self.n = n
        self.arr = (N.ConvLaunch * n)()
        self.keep = rec.keep
        self.in_slots, self.out_slots = [], []
        pin, pout = x_in.data_ptr(), out.data_ptr()
        for i, (_, launch) in enumerate(rec.launches):
            self.arr[i] = launch  # a copy: `run` patches the plan's own descriptors
            c = self.arr[i]
            for name in ("x", "x2", "residual"):
                if getattr(c, name) == pin:
                    self.in_slots.append((i, name))
            for name in ("y", "head_out"):
                if getattr(c, name) == pout:
                    self.out_slots.append((i, name))
        if not self.in_slots or not self.out_slots:
            raise RuntimeError("conv plan: input / output tensor not found among the recorded launches")

    def run(self, x_in, out):
        pin, pout = x_in.data_ptr(), out.data_ptr()
        for i, name in self.in_slots:
            setattr(self.arr[i], name, pin)
        for i, name in self.out_slots:
            setattr(self.arr[i], name, pout)
        if _timer is not None and _timer.last_conv and self.n > 1:
            N.check(N.lib().lss_conv2d_sequence(self.arr, self.n - 1, N.stream()), "lss_conv2d_sequence")
            last = ctypes.byref(self.arr, (self.n - 1) * ctypes.sizeof(self.arr[0]))  # &arr[n - 1]
            with _timed("conv_plan_last", coarse=True):
                N.check(N.lib().lss_conv2d_sequence(last, 1, N.stream()), "lss_conv2d_sequence")
            return
        N.check(N.lib().lss_conv2d_sequence(self.arr, self.n, N.stream()), "lss_conv2d_sequence")


class SplatWorkspace:
    """Index buffers of one (B,N,D,fH,fW | X,Y,Z) problem, reused across steps.

    vox_count and cursor obey the K4 contract: zero on entry, zero on return, so
    they are zero-filled exactly once, here."""

    def __init__(self, P, nvox, device):
        self.P, self.nvox = P, nvox
        self.voxel = torch.empty(P, dtype=torch.int32, device=device)
        self.vox_count = torch.zeros(nvox, dtype=torch.int32, device=device)
        self.vox_list = torch.empty(nvox, 2, dtype=torch.int32, device=device)
        self.entries = torch.empty(P, 2, dtype=torch.int32, device=device)  # {point id, depth weight}
        self.cursor = torch.zeros(1, dtype=torch.int32, device=device)
        self._direct = {}

    def direct_buffer(self, dims, nx):
        """The larger entry workspace of the two-launch (direct) region pipeline (lss_lift_splat_direct_bytes): fixed-
        capacity per-region buckets, 8 KiB per region (20 MB at batch 4, 200 x 200); None where the region pipeline
        does not apply or with LSS_SPLAT_DIRECT=0.  Allocated on first use (a warm-up step, never inside a capture)."""
        key = (tuple(dims), tuple(nx))
        if key not in self._direct:
            B, Ncam, D, fH, fW, C = dims
            X, Y, Z = nx
            n = 0 if os.environ.get("LSS_SPLAT_DIRECT") == "0" else \
                int(N.lib().lss_lift_splat_direct_bytes(B, Ncam, D, fH, fW, C, X, Y, Z))
            self._direct[key] = torch.empty(n, dtype=torch.uint8, device=self.voxel.device) if n else None
        return self._direct[key]


def _check_geometry(frustum, dx, bx, dims, calib_dev=None):
    """frustum (D,fH,fW,3), dx / bx (3,) and - unless the calibration travels as a host buffer - the per-camera
    tensors calib_dev = (inv_post_rots, post_trans, combine, trans): (B,N,3,3) / (B,N,3)."""
    B, Ncam, D, fH, fW = dims[:5]
    _f32c(frustum, "frustum", (D, fH, fW, 3))
    if calib_dev is not None:
        inv_post_rots, post_trans, combine, trans = calib_dev
        _f32c(inv_post_rots, "inv_post_rots", (B, Ncam, 3, 3))
        _f32c(combine, "combine", (B, Ncam, 3, 3))
        _f32c(post_trans, "post_trans", (B, Ncam, 3))
        _f32c(trans, "trans", (B, Ncam, 3))
    _f32c(dx, "dx", (3,))
    _f32c(bx, "bx", (3,))


def _check_depthnet(x, weight, bias, dims):
    """x (B*N,Cin,fH,fW), weight (D+C,Cin[,1,1]), bias (D+C).  Returns (x, 2-D weight, bias)."""
    B, Ncam, D, fH, fW, C = dims
    Cin = x.shape[1]
    _f32c(x, "x", (B * Ncam, Cin, fH, fW))
    w2 = weight.reshape(weight.shape[0], -1)
    _f32c(w2, "depthnet.weight", (D + C, Cin))
    _f32c(bias, "depthnet.bias", (D + C,))
    return x, w2, bias


def _check_workspace(ws, dims, nx):
    B, Ncam, D, fH, fW = dims[:5]
    X, Y, Z = nx
    P = B * Ncam * D * fH * fW
    if ws.P != P or ws.nvox != B * X * Y * Z:
        raise ValueError("workspace sized for P=%d nvox=%d, problem has P=%d nvox=%d" % (ws.P, ws.nvox, P, B * X * Y * Z))


def _alloc_bev(dims, nx, layout, device):
    """BEV storage for `layout` and its LOGICAL (B, Z*C, X, Y) view: contiguous for NCHW_F32, channels_last strides for
    NHWC_*."""
    B, C = dims[0], dims[5]
    X, Y, Z = nx
    if layout == BEV_NCHW_F32:
        bev = torch.empty(B, Z * C, X, Y, dtype=torch.float32, device=device)
        return bev, bev
    bev = torch.empty(B, X, Y, Z * C, dtype=torch.float32 if layout == BEV_NHWC_F32 else torch.bfloat16, device=device)
    return bev, bev.permute(0, 3, 1, 2)


def _lift_splat_run(what, ws, dims, nx, layout, math, frustum, dx, bx, calib_dev=None, calib_host=None, depthnet=None,
                    heads=None):
    """Fill one lss_lift_splat_desc_t (include/lss_hip.h) for any of the three forms of the fused lift-splat call and
    run it.  depthnet = (x, 2-D weight, bias): depth / feat are allocated here; heads = (depth, feat): they are inputs.
    Returns (bev as its logical view, depth, feat)."""
    B, Ncam, D, fH, fW, C = dims
    _check_workspace(ws, dims, nx)
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    d = N.LiftSplatDesc()
    if depthnet is not None:
        x, w, bias = depthnet
        d.x, d.w, d.bias, d.Cin = P(x), P(w), P(bias), x.shape[1]
        depth = torch.empty(B * Ncam, D, fH, fW, dtype=torch.float32, device=x.device)
        feat = torch.empty(B * Ncam, fH, fW, C, dtype=torch.float32, device=x.device)
    else:
        depth, feat = heads
    bev, out = _alloc_bev(dims, nx, layout, feat.device)
    d.frustum, d.dx, d.bx = P(frustum), P(dx), P(bx)
    if calib_host is not None:
        d.calib_host = calib_host.data_ptr()
    else:
        d.inv_post_rots, d.post_trans, d.combine, d.trans = (P(t) for t in calib_dev)
    d.voxel, d.vox_count, d.vox_list = P(ws.voxel), P(ws.vox_count), P(ws.vox_list)
    d.entries, d.cursor = P(ws.entries), P(ws.cursor)
    direct = ws.direct_buffer(dims, nx)
    d.direct_entries = P(direct)
    d.direct_bytes = 0 if direct is None else direct.numel()
    d.depth, d.feat, d.bev = P(depth), P(feat), P(bev)
    d.B, d.N, d.D, d.fH, d.fW, d.C = dims
    d.X, d.Y, d.Z = nx
    d.layout, d.math = layout, math
    N.check(N.lib().lss_lift_splat_forward_desc(ctypes.byref(d), N.stream()), what)
    return out, depth, feat


def points_to_voxels(frustum, inv_post_rots, post_trans, combine, trans, dx, bx, nx, ws,
                     want_geom=False, histogram=True):
    """K3.  frustum (D,fH,fW,3); per-camera tensors (B,N,3,3)/(B,N,3); nx = (X,Y,Z) ints.
    Fills ws.voxel (+ ws.vox_count histogram); returns geom (B,N,D,fH,fW,3) or None."""
    D, fH, fW, _ = frustum.shape
    B, Ncam = inv_post_rots.shape[:2]
    X, Y, Z = nx
    dims = (B, Ncam, D, fH, fW)
    _check_geometry(frustum, dx, bx, dims, (inv_post_rots, post_trans, combine, trans))
    _check_workspace(ws, dims, nx)
    geom = torch.empty(B, Ncam, D, fH, fW, 3, dtype=torch.float32, device=frustum.device) if want_geom else None
    N.check(N.lib().lss_points_to_voxels(
        N.ptr(frustum), N.ptr(inv_post_rots), N.ptr(post_trans), N.ptr(combine), N.ptr(trans),
        N.ptr(dx), N.ptr(bx), B, Ncam, D, fH, fW, X, Y, Z, N.ptr(ws.voxel),
        N.ptr(ws.vox_count) if histogram else None, N.ptr(geom), N.stream()), "lss_points_to_voxels")
    return geom


def geom_to_voxels(geom, dx, bx, nx, B, ws, histogram=True):
    """API-compat half of K3: geom (..., 3) fp32 with B samples of equal point count."""
    _f32c(geom, "geom")
    P = geom.numel() // 3
    X, Y, Z = nx
    if geom.shape[-1] != 3 or P % B != 0 or ws.P != P or ws.nvox != B * X * Y * Z:
        raise ValueError("geom / workspace shape mismatch")
    N.check(N.lib().lss_geom_to_voxels(N.ptr(geom), N.ptr(_f32c(dx, "dx", (3,))), N.ptr(_f32c(bx, "bx", (3,))),
                                       B, P // B, X, Y, Z, N.ptr(ws.voxel),
                                       N.ptr(ws.vox_count) if histogram else None, N.stream()),
            "lss_geom_to_voxels")


def bucket_points(ws, depth=None, D=1, HW=1):
    """K4 on a workspace whose voxel/vox_count were filled by K3.  `depth` = K2's
    (BN,D,fH,fW) tensor (its flat index is the point id); None = unit weights with the
    points taken as D = HW = 1 rows (pre-lifted inputs)."""
    if depth is not None:
        _f32c(depth, "depth")
        if depth.numel() != ws.P or depth.dim() != 4:
            raise ValueError("depth must be (BN,D,fH,fW) with %d elements" % ws.P)
        D, HW = depth.shape[1], depth.shape[2] * depth.shape[3]
    N.check(N.lib().lss_bucket_points(N.ptr(ws.voxel), N.ptr(depth), ws.P, D, HW, ws.nvox, N.ptr(ws.vox_count),
                                      N.ptr(ws.vox_list), N.ptr(ws.entries), N.ptr(ws.cursor),
                                      N.stream()), "lss_bucket_points")


def depthnet_softmax(x, weight, bias, D, C, math=DT_F32):
    """K2.  x (BN,Cin,fH,fW) fp32 NCHW; weight (D+C,Cin,1,1) or (D+C,Cin); bias (D+C).
    Returns depth (BN,D,fH,fW) and feat (BN,fH,fW,C) (channels-last rows)."""
    BN, Cin, fH, fW = x.shape
    _f32c(x, "x")
    w2 = weight.reshape(weight.shape[0], -1)
    _f32c(w2, "depthnet.weight", (D + C, Cin))
    _f32c(bias, "depthnet.bias", (D + C,))
    depth = torch.empty(BN, D, fH, fW, dtype=torch.float32, device=x.device)
    feat = torch.empty(BN, fH, fW, C, dtype=torch.float32, device=x.device)
    N.check(N.lib().lss_depthnet_softmax_fwd(N.ptr(x), N.ptr(w2), N.ptr(bias), BN, Cin, fH * fW, D, C,
                                             N.ptr(depth), N.ptr(feat), math, N.stream()),
            "lss_depthnet_softmax_fwd")
    return depth, feat


def camencode_v2(hidden, w_depth, b_depth, D, c3=None, w_feat=None, b_feat=None, softmax=True, math=None):
    """K2v.  hidden (BN,fH,fW,Cd) NHWC fp32|bf16; w_depth (D,Cd[,1,1]); optional c3
    (BN,Cf,fH,fW) fp32 NCHW with w_feat (C,Cf[,1,1]) / b_feat.  Returns depth
    (BN,D,fH,fW) (probabilities, or raw logits with softmax=False) and feat
    (BN,fH,fW,C) or None.  math: DT_F32 (exact fp32 FMA chains) or DT_BF16 (bf16 MFMA, fp32
    accumulate); default = the hidden map's own precision when the shapes allow."""
    BN, fH, fW, Cd = hidden.shape
    if not hidden.is_contiguous() or hidden.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("hidden must be contiguous NHWC fp32/bf16")
    dt = DT_F32 if hidden.dtype == torch.float32 else DT_BF16
    wd = w_depth.reshape(w_depth.shape[0], -1)
    _f32c(wd, "w_depth", (D, Cd))
    _f32c(b_depth, "b_depth", (D,))
    dev = hidden.device
    depth = torch.empty(BN, D, fH, fW, dtype=torch.float32, device=dev)
    if c3 is not None:
        _f32c(c3, "c3")
        if c3.shape[0] != BN or tuple(c3.shape[2:]) != (fH, fW):
            raise ValueError("c3 %s does not match hidden %s" % (tuple(c3.shape), tuple(hidden.shape)))
        Cf = c3.shape[1]
        wf = w_feat.reshape(w_feat.shape[0], -1)
        C = wf.shape[0]
        _f32c(wf, "w_feat", (C, Cf))
        _f32c(b_feat, "b_feat", (C,))
        feat = torch.empty(BN, fH, fW, C, dtype=torch.float32, device=dev)
        args = (N.ptr(c3), N.ptr(wf), N.ptr(b_feat), Cf)
    else:
        C, feat, args = 0, None, (None, None, None, 0)
    if math is None:
        math = DT_BF16 if (dt == DT_BF16 and Cd % 128 == 0 and (C == 0 or args[3] % 128 == 0)) else DT_F32
    with _timed("camencode_v2"):
        N.check(N.lib().lss_camencode_v2_fwd(N.ptr(hidden), dt, N.ptr(wd), N.ptr(b_depth), Cd, *args, BN,
                                             fH * fW, D, C, 1 if softmax else 0, math, N.ptr(depth),
                                             N.ptr(feat) if feat is not None else None, N.stream()),
                "lss_camencode_v2_fwd")
    return depth, feat


def depth_fuse_softmax(d3, d4, w_fusion, scale, shift):
    """MultiScaleDepthNet tail: d3 (BN,D,H,W), d4 (BN,D,H4,W4) raw logits ->
    softmax(relu(scale * fusion([d3, up(d4)]) + shift)) (BN,D,H,W)."""
    BN, D, H, W = d3.shape
    _f32c(d3, "d3")
    _f32c(d4, "d4")
    if d4.shape[0] != BN or d4.shape[1] != D:
        raise ValueError("d4 %s does not match d3 %s" % (tuple(d4.shape), tuple(d3.shape)))
    w2 = w_fusion.reshape(w_fusion.shape[0], -1)
    _f32c(w2, "w_fusion", (D, 2 * D))
    _f32c(scale, "scale", (D,))
    _f32c(shift, "shift", (D,))
    depth = torch.empty_like(d3)
    with _timed("depth_fuse_softmax"):
        N.check(N.lib().lss_depth_fuse_softmax_fwd(N.ptr(d3), N.ptr(d4), N.ptr(w2), N.ptr(scale), N.ptr(shift),
                                                   BN, D, H, W, d4.shape[2], d4.shape[3], N.ptr(depth),
                                                   N.stream()), "lss_depth_fuse_softmax_fwd")
    return depth


_fuse_train_ws = {}


def _depth_fuse_train_args(d3, d4, w_fusion):
    """Shape checks shared by both directions of the training tail; returns (dims, w (D, 2D), cached workspace)."""
    if d3.dim() != 4 or d4.dim() != 4:
        raise ValueError("d3 and d4 must be (BN, D, H, W) logits, got %s and %s" % (tuple(d3.shape), tuple(d4.shape)))
    BN, D, H, W = d3.shape
    _f32c(d3, "d3")
    _f32c(d4, "d4")
    if d4.shape[0] != BN or d4.shape[1] != D:
        raise ValueError("d4 %s does not match d3 %s" % (tuple(d4.shape), tuple(d3.shape)))
    if BN * H * W < 2:  # nn.BatchNorm2d's own refusal, in its words
        raise ValueError("Expected more than 1 value per channel when training, got input size %s"
                         % (torch.Size((BN, D, H, W)),))
    w2 = w_fusion.reshape(w_fusion.shape[0], -1)
    _f32c(w2, "w_fusion", (D, 2 * D))
    nbytes = N.lib().lss_depth_fuse_train_workspace_bytes(BN, D, H, W)
    if nbytes == 0:
        raise ValueError("the training tail takes D <= 64 and fewer than 2^31 pixels (got BN=%d D=%d H=%d W=%d)"
                         % (BN, D, H, W))
    ws = _cached_ws(_fuse_train_ws, (BN, D, H, W, str(d3.device)), nbytes, d3.device)
    return (BN, D, H, W, d4.shape[2], d4.shape[3]), w2, ws


def depth_fuse_train_fwd(d3, d4, w_fusion, bias, gamma, beta, running_mean, running_var, momentum, eps):
    """MultiScaleDepthNet's tail in training mode (lss_depth_fuse_train_fwd): d3 (BN,D,H,W), d4 (BN,D,H4,W4) fp32
    logits -> z = fusion([d3, up(d4)]) + bias, u = relu(BatchNorm_train(z)) (both (BN,D,H,W) fp32), save_mean,
    save_invstd (D); running_mean / running_var are updated in place like nn.BatchNorm2d's."""
    dims, w2, ws = _depth_fuse_train_args(d3, d4, w_fusion)
    D = dims[1]
    for t, nm in ((bias, "bias"), (gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"),
                  (running_var, "running_var")):
        _f32c(t, nm, (D,))
    z, u = torch.empty_like(d3), torch.empty_like(d3)
    mean = torch.empty(D, dtype=torch.float32, device=d3.device)
    invstd = torch.empty(D, dtype=torch.float32, device=d3.device)
    with _timed("depth_fuse_train_fwd"):
        N.check(N.lib().lss_depth_fuse_train_fwd(N.ptr(d3), N.ptr(d4), N.ptr(w2), N.ptr(bias), N.ptr(gamma),
                                                 N.ptr(beta), N.ptr(running_mean), N.ptr(running_var),
                                                 float(momentum), float(eps), *dims, N.ptr(ws), ws.numel(), N.ptr(z),
                                                 N.ptr(u), N.ptr(mean), N.ptr(invstd), N.stream()),
                "lss_depth_fuse_train_fwd")
    return z, u, mean, invstd


def depth_fuse_train_bwd(du, u, z, d3, d4, w_fusion, gamma, mean, invstd):
    """Backward of `depth_fuse_train_fwd` (lss_depth_fuse_train_bwd): returns (d(d3), d(d4), dW like w_fusion, dgamma,
    dbeta), all fp32 and bit-reproducible; the conv bias in front of the BatchNorm has gradient zero."""
    dims, w2, ws = _depth_fuse_train_args(d3, d4, w_fusion)
    D = dims[1]
    for t, nm in ((du, "du"), (u, "u"), (z, "z")):
        _f32c(t, nm, d3.shape)
    for t, nm in ((gamma, "gamma"), (mean, "mean"), (invstd, "invstd")):
        _f32c(t, nm, (D,))
    dd3, dd4 = torch.empty_like(d3), torch.empty_like(d4)
    dw = torch.empty(w_fusion.shape, dtype=torch.float32, device=d3.device)
    dgamma = torch.empty(D, dtype=torch.float32, device=d3.device)
    dbeta = torch.empty(D, dtype=torch.float32, device=d3.device)
    with _timed("depth_fuse_train_bwd"):
        N.check(N.lib().lss_depth_fuse_train_bwd(N.ptr(du), N.ptr(u), N.ptr(z), N.ptr(d3), N.ptr(d4), N.ptr(w2),
                                                 N.ptr(gamma), N.ptr(mean), N.ptr(invstd), *dims, N.ptr(ws),
                                                 ws.numel(), N.ptr(dd3), N.ptr(dd4), N.ptr(dw), N.ptr(dgamma),
                                                 N.ptr(dbeta), N.stream()), "lss_depth_fuse_train_bwd")
    return dd3, dd4, dw, dgamma, dbeta


def lift_splat_fwd(feat, ws, dims, nx, layout=BEV_NCHW_F32, tag="lift_splat_fwd"):
    """K5/K6 on a bucketed workspace (depth weights already sit in ws.entries).
    dims = (B,N,D,fH,fW,C).  Returns the BEV tensor with LOGICAL shape
    (B, Z*C, X, Y): contiguous for NCHW_F32, channels_last strides for NHWC_*."""
    B, Ncam, D, fH, fW, C = dims
    X, Y, Z = nx
    _f32c(feat, "feat")
    if feat.numel() != B * Ncam * fH * fW * C:
        raise ValueError("feat size does not match dims %s" % (dims,))
    _check_workspace(ws, dims, nx)
    bev, out = _alloc_bev(dims, nx, layout, feat.device)
    with _timed(tag):
        N.check(N.lib().lss_lift_splat_fwd(N.ptr(feat), N.ptr(ws.vox_list), N.ptr(ws.entries),
                                           B, Ncam, D, fH, fW, C, X, Y, Z, N.ptr(bev), layout, N.stream()),
                "lss_lift_splat_fwd")
    return out


def lift_splat_forward(frustum, inv_post_rots, post_trans, combine, trans, dx, bx, x, weight, bias, ws, dims, nx,
                       layout=BEV_NCHW_F32, math=DT_F32):
    """K3 -> K2 -> K4 -> K5 with ONE native call (inference path).  Returns (bev, depth, feat)."""
    calib_dev = (inv_post_rots, post_trans, combine, trans)
    _check_geometry(frustum, dx, bx, dims, calib_dev)
    return _lift_splat_run("lss_lift_splat_forward_desc", ws, dims, nx, layout, math, frustum, dx, bx, calib_dev=calib_dev,
                           depthnet=_check_depthnet(x, weight, bias, dims))


def ffn_fused(x, w1, b1, w2, b2, ln=None):
    """y = x + b2 + W2 . gelu(W1 . x + b1) in one launch (transformer FFN, erf GELU).
    x (..., 256) bf16 contiguous; w1 (F, 256) / w2 (256, F) bf16 (packed 1x1 weights are accepted as
    (1, N, K)); b1 (F), b2 (256) fp32.  Returns fp32 of x's shape (the pre-LayerNorm sum), or - with
    ln = (gamma, beta, eps) - LayerNorm(y) * gamma + beta in bf16, normalised in the kernel's epilogue."""
    w1 = w1.reshape(w1.shape[-2], w1.shape[-1])
    w2 = w2.reshape(w2.shape[-2], w2.shape[-1])
    F, Dm = w1.shape
    if x.dtype != torch.bfloat16 or w1.dtype != torch.bfloat16 or w2.dtype != torch.bfloat16:
        raise ValueError("ffn_fused: bf16 operands")
    if not (x.is_contiguous() and w1.is_contiguous() and w2.is_contiguous()) or x.shape[-1] != Dm \
            or tuple(w2.shape) != (Dm, F):
        raise ValueError("ffn_fused: x (...,%d), w1 (F,%d), w2 (%d,F) contiguous" % (Dm, Dm, Dm))
    _f32c(b1, "b1", (F,))
    _f32c(b2, "b2", (Dm,))
    M = x.numel() // Dm
    gamma = beta = y = y_ln = None
    eps = 0.0
    if ln is None:
        y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    else:
        gamma, beta, eps = ln
        _f32c(gamma, "ln.gamma", (Dm,))
        _f32c(beta, "ln.beta", (Dm,))
        y_ln = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    with _timed("ffn_fused"):
        N.check(N.lib().lss_ffn_fused_fwd(N.ptr(x), N.ptr(w1), N.ptr(b1), N.ptr(w2), N.ptr(b2), M, Dm, F, N.ptr(y),
                                          N.ptr(gamma), N.ptr(beta), float(eps), N.ptr(y_ln), N.stream()),
                "lss_ffn_fused_fwd")
    return y if ln is None else y_ln


def linear_res_ln(x, w, bias, residual, ln=None):
    """x . W^T + bias + residual for a 256 -> 256 layer, fp32 - or, with ln = (gamma, beta, eps), its LayerNorm
    in bf16 without the fp32 sum ever being written.  x, residual (..., 256) bf16; w (256, 256) bf16 (packed
    1x1 weights (1, N, K) accepted); bias (256) fp32."""
    w = w.reshape(w.shape[-2], w.shape[-1])
    Dm = x.shape[-1]
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or residual.dtype != torch.bfloat16:
        raise ValueError("linear_res_ln: bf16 operands")
    if not (x.is_contiguous() and w.is_contiguous() and residual.is_contiguous()) or tuple(w.shape) != (Dm, Dm) \
            or residual.shape != x.shape:
        raise ValueError("linear_res_ln: x, residual (...,%d) and w (%d,%d) contiguous" % (Dm, Dm, Dm))
    _f32c(bias, "bias", (Dm,))
    M = x.numel() // Dm
    gamma = beta = y = y_ln = None
    eps = 0.0
    if ln is None:
        y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    else:
        gamma, beta, eps = ln
        _f32c(gamma, "ln.gamma", (Dm,))
        _f32c(beta, "ln.beta", (Dm,))
        y_ln = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    with _timed("linear_res_ln"):
        N.check(N.lib().lss_linear_res_ln_fwd(N.ptr(x), N.ptr(w), N.ptr(bias), N.ptr(residual), M, Dm, N.ptr(y),
                                              N.ptr(gamma), N.ptr(beta), float(eps), N.ptr(y_ln), N.stream()),
                "lss_linear_res_ln_fwd")
    return y if ln is None else y_ln


HOSTCAL_MAX_CAMS = 36


def lift_splat_from_heads(frustum, inv_post_rots, post_trans, combine, trans, dx, bx, depth, feat, ws, dims, nx,
                          layout=BEV_NCHW_F32):
    """Geometry + bucketing + splat of depth (B*N, D, fH, fW) / context (B*N, fH, fW, C) tensors that other kernels
    produced (the vovnet depth heads + CamEncodeV2) with ONE native call; region-bucketed pipeline when the problem
    fits it.  Returns the BEV grid (logical (B, Z*C, X, Y))."""
    B, Ncam, D, fH, fW, C = dims
    calib_dev = (inv_post_rots, post_trans, combine, trans)
    _check_geometry(frustum, dx, bx, dims, calib_dev)
    _f32c(depth, "depth", (B * Ncam, D, fH, fW))
    _f32c(feat, "feat")
    if feat.numel() != B * Ncam * fH * fW * C or C not in (64, 128):
        raise ValueError("feat must hold (B*N*fH*fW, C) context rows with C in (64, 128)")
    return _lift_splat_run("lss_lift_splat_forward_desc (from heads)", ws, dims, nx, layout, DT_F32, frustum, dx, bx,
                           calib_dev=calib_dev, heads=(depth, feat))[0]


def lift_splat_forward_hostcal(frustum, calib_host, dx, bx, x, weight, bias, ws, dims, nx, layout=BEV_NCHW_F32):
    """lift_splat_forward with the calibration as ONE CPU fp32 buffer of B*N*24 floats
    ([inv_post_rots | combine | post_trans | trans] = data.CalibrationPack.buffer): it is read during the
    call and rides in the kernel arguments - no H2D copy.  B*N <= HOSTCAL_MAX_CAMS; f32 depthnet math."""
    B, Ncam = dims[:2]
    if calib_host.is_cuda or calib_host.dtype != torch.float32 or not calib_host.is_contiguous() \
            or calib_host.numel() != B * Ncam * 24 or B * Ncam > HOSTCAL_MAX_CAMS:
        raise ValueError("calib_host must be a contiguous CPU fp32 buffer of B*N*24 floats (B*N <= %d)" % HOSTCAL_MAX_CAMS)
    _check_geometry(frustum, dx, bx, dims)
    return _lift_splat_run("lss_lift_splat_forward_desc (host calibration)", ws, dims, nx, layout, DT_F32, frustum, dx, bx,
                           calib_host=calib_host, depthnet=_check_depthnet(x, weight, bias, dims))


def lift_splat_bwd(grad_bev, voxel, depth, feat, dims, nx):
    """K7.  grad_bev logical (B, Z*C, X, Y): fp32 contiguous or channels_last, or bf16 channels_last (the gradient a
    bf16 stem hands back: read as it is, no fp32 copy).  Returns g_logits (BN, D+C, fH, fW)."""
    B, Ncam, D, fH, fW, C = dims
    X, Y, Z = nx
    if tuple(grad_bev.shape) != (B, Z * C, X, Y):
        raise ValueError("grad_bev must be (B, Z*C, X, Y)")
    if grad_bev.dtype == torch.bfloat16 and grad_bev.is_contiguous(memory_format=torch.channels_last):
        layout = BEV_NHWC_BF16
    else:
        if grad_bev.dtype != torch.float32:
            grad_bev = grad_bev.float()
        if grad_bev.is_contiguous():
            layout = BEV_NCHW_F32
        elif grad_bev.is_contiguous(memory_format=torch.channels_last):
            layout = BEV_NHWC_F32
        else:
            grad_bev = grad_bev.contiguous()
            layout = BEV_NCHW_F32
    g_logits = torch.empty(B * Ncam, D + C, fH, fW, dtype=torch.float32, device=grad_bev.device)
    N.check(N.lib().lss_lift_splat_bwd(N.ptr(grad_bev), layout, N.ptr(voxel), N.ptr(depth), N.ptr(feat),
                                       B, Ncam, D, fH, fW, C, X, Y, Z, N.ptr(g_logits), N.stream()),
            "lss_lift_splat_bwd")
    return g_logits


def pointwise_conv_bwd_ok(BN, K, M, HW):
    """True when `pointwise_conv_bwd` accepts the shape (K % 64 == 0, K <= 1024, M <= 192, HW >= 1)."""
    return bool(N.lib().lss_pointwise_conv_bwd_ok(int(BN), int(K), int(M), int(HW)))


def pointwise_conv_bwd(g, x, w, layout="nchw", g_ch_off=0, M=None, want_dx=True, want_dw=True, want_db=True):
    """K10: backward of a 1x1 conv y = w x + bias (lss_pointwise_conv_bwd).
    g  fp32 output gradient (BN, Mg, *spatial), channel-major: pixel stride 1, channel stride HW, any image stride
       >= Mg * HW (a channel slice of a wider tensor is read in place); channels [g_ch_off, g_ch_off + M) are used
       (M defaults to Mg - g_ch_off);
    x  layout "nchw": (BN, K, *spatial) fp32; "nhwc": (BN, *spatial, K) fp32 | bf16, contiguous;
    w  (M, K[, 1, 1]) fp32.
    Returns (dx like x | None, dw like w | None, db (M) | None); dw and db are bit-reproducible."""
    if layout not in ("nchw", "nhwc"):
        raise ValueError("layout must be 'nchw' or 'nhwc'")
    if g.dim() < 3 or g.dtype != torch.float32:
        raise ValueError("g must be an fp32 (BN, M, *spatial) tensor, got %s %s" % (g.dtype, tuple(g.shape)))
    BN, Mg = g.shape[0], g.shape[1]
    spatial = tuple(g.shape[2:])
    HW = 1
    for v in spatial:
        HW *= v
    M = Mg - g_ch_off if M is None else M
    if g_ch_off < 0 or M <= 0 or g_ch_off + M > Mg:
        raise ValueError("channels [%d, %d) are not inside g's %d" % (g_ch_off, g_ch_off + M, Mg))
    w2 = w.reshape(w.shape[0], -1)
    if w2.dtype != torch.float32 or w2.shape[0] != M or not w.is_contiguous():  # (dw is written dense, in w's shape)
        raise ValueError("w must be contiguous fp32 (%d, K[, 1, 1]), got %s %s" % (M, w.dtype, tuple(w.shape)))
    K = w2.shape[1]
    want = (BN, K) + spatial if layout == "nchw" else (BN,) + spatial + (K,)
    ok_dt = (torch.float32,) if layout == "nchw" else (torch.float32, torch.bfloat16)
    if x.dtype not in ok_dt or tuple(x.shape) != want or not x.is_contiguous():
        raise ValueError("x must be contiguous %s of %s, got %s %s"
                         % (want, " | ".join(str(d) for d in ok_dt), tuple(x.shape), x.dtype))
    if not pointwise_conv_bwd_ok(BN, K, M, HW):
        raise ValueError("pointwise_conv_bwd needs K %% 64 == 0, K <= 1024, M <= 192, BN <= 4096, BN * HW <= 2^22 "
                         "(got BN=%d, K=%d, M=%d, HW=%d)" % (BN, K, M, HW))
    if not (g.is_cuda and x.is_cuda and w2.is_cuda):
        raise ValueError("g, x and w must be GPU tensors")
    # channel-major with unit pixel stride; anything else (a transposed gradient autograd made contiguous its own way)
    # is copied once
    gs = g
    if not _flat_ok(g) or (Mg > 1 and g.stride(1) != HW) or (BN > 1 and g.stride(0) < Mg * HW):
        gs = g.contiguous()
    g_bstride = gs.stride(0) if BN > 1 else Mg * HW
    layout_id = PW_NCHW_F32 if layout == "nchw" else (PW_NHWC_F32 if x.dtype == torch.float32 else PW_NHWC_BF16)
    dev = x.device
    dx = torch.empty_like(x) if want_dx else None
    dw = torch.empty_like(w) if want_dw else None
    db = torch.empty(M, dtype=torch.float32, device=dev) if want_db else None
    ws, nbytes = None, 0
    if want_dw or want_db:
        nbytes = N.lib().lss_pointwise_conv_bwd_workspace_bytes(BN, K, M, HW)
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
    with _timed("pointwise_conv_bwd"):
        N.check(N.lib().lss_pointwise_conv_bwd(N.ptr(gs), g_ch_off, g_bstride, N.ptr(x), layout_id, N.ptr(w2), BN, K, M,
                                               HW, N.ptr(ws), nbytes, N.ptr(dx), N.ptr(dw), N.ptr(db), N.stream()),
                "lss_pointwise_conv_bwd")
    return dx, dw, db


def _flat_ok(t):
    """True when the trailing (spatial) dims of t can be flattened without a copy."""
    exp = 1
    for size, stride in zip(reversed(t.shape[2:]), reversed(t.stride()[2:])):
        if size != 1 and stride != exp:
            return False
        exp *= size
    return True


def segmented_sum(x, seg_start):
    """x (K,C) fp32, seg_start (M+1) int32 -> (M,C)."""
    _f32c(x, "x")
    M = seg_start.numel() - 1
    y = torch.empty(M, x.shape[1], dtype=torch.float32, device=x.device)
    if M > 0:
        N.check(N.lib().lss_segmented_sum(N.ptr(x), N.ptr(seg_start), M, x.shape[1], N.ptr(y), N.stream()),
                "lss_segmented_sum")
    return y


_TORCH_DT = {DT_F32: torch.float32, DT_BF16: torch.bfloat16}


def add_pos(x, pos):
    """q = x + pos: x (B, ..., 256) token rows in fp32|bf16, pos (T, 256) fp32 with T = tokens per sample."""
    if not x.is_contiguous() or x.dtype not in _DT:
        raise ValueError("x must be contiguous fp32/bf16")
    _f32c(pos, "pos")
    B, C = x.shape[0], x.shape[-1]
    T = x.numel() // (B * C)
    if tuple(pos.shape) != (T, C):
        raise ValueError("pos %s does not match %d tokens x %d channels" % (tuple(pos.shape), T, C))
    q = torch.empty_like(x)
    with _timed("add_pos"):
        N.check(N.lib().lss_add_pos_fwd(N.ptr(x), N.ptr(pos), B, T, C, _DT[x.dtype], N.ptr(q), N.stream()), "lss_add_pos_fwd")
    return q


def deform_attn(value, offsets_logits, ref_x, ref_y, n_heads=8, n_points=8, token_bias=None):
    """value fp32|bf16: (B,H,W,256) NHWC, or head-major (B,8,H*W,32) (conv2d_nhwc(head_major=True));
    offsets_logits (B,H,W,192) fp32; token_bias (H*W,192) fp32 or None (per-token addend shared by
    all samples) -> (B,H,W,256) NHWC in value's dtype."""
    B, H, W = offsets_logits.shape[:3]
    C = n_heads * 32
    if tuple(value.shape) == (B, H, W, C):
        layout = VALUE_NHWC
    elif tuple(value.shape) == (B, n_heads, H * W, 32):
        layout = VALUE_HEAD_MAJOR
    else:
        raise ValueError("value %s is neither (B,H,W,%d) nor (B,%d,H*W,32)" % (tuple(value.shape), C, n_heads))
    if not value.is_contiguous() or value.dtype not in _DT:
        raise ValueError("value must be contiguous fp32/bf16")
    _f32c(offsets_logits, "offsets_logits", (B, H, W, n_heads * n_points * 3))
    _f32c(ref_x, "ref_x", (W,))
    _f32c(ref_y, "ref_y", (H,))
    if token_bias is not None:
        _f32c(token_bias, "token_bias", (H * W, n_heads * n_points * 3))
    out = torch.empty(B, H, W, C, dtype=value.dtype, device=value.device)
    with _timed("deform_attn"):
        N.check(N.lib().lss_deform_attn_fwd(N.ptr(value), layout, N.ptr(offsets_logits), N.ptr(token_bias), N.ptr(ref_x),
                                            N.ptr(ref_y), B, H, W, n_heads, n_points, C, _DT[value.dtype],
                                            N.ptr(out), N.stream()), "lss_deform_attn_fwd")
    return out


def _ref_pts_arg(ref_pts, B, T):
    """(B, T, 2) fp32 GPU reference points -> (tensor whose storage is read, sample stride in floats).  A batch
    stride of 0 (torch's expand()) is passed through as is; other layouts are made contiguous."""
    if ref_pts.dtype != torch.float32 or not ref_pts.is_cuda or ref_pts.dim() != 3 \
            or tuple(ref_pts.shape[1:]) != (T, 2) or ref_pts.shape[0] not in (1, B):
        raise ValueError("ref_pts must be fp32 GPU (B, %d, 2), got %s %s %s"
                         % (T, ref_pts.dtype, ref_pts.device, tuple(ref_pts.shape)))
    if ref_pts.stride(2) != 1 or ref_pts.stride(1) != 2 or ref_pts.storage_offset() % 2:
        ref_pts = ref_pts.contiguous()
    return ref_pts, (0 if ref_pts.shape[0] == 1 else ref_pts.stride(0))


def deform_attn_pts(value, offsets_logits, ref_pts, H, W):
    """Deformable-attention core with per-token reference points (lss_deform_attn_pts_fwd).
    value (B, H*W, 256) fp32; offsets_logits (B, H*W, 192) fp32; ref_pts (B, H*W, 2) fp32 (batch stride 0 allowed)
    -> (B, H*W, 256) fp32."""
    B = value.shape[0]
    _f32c(value, "value", (B, H * W, 256))
    _f32c(offsets_logits, "offsets_logits", (B, H * W, 192))
    ref_pts, rstride = _ref_pts_arg(ref_pts, B, H * W)
    out = torch.empty(B, H * W, 256, dtype=torch.float32, device=value.device)
    with _timed("deform_attn"):
        N.check(N.lib().lss_deform_attn_pts_fwd(N.ptr(value), N.ptr(offsets_logits), N.ptr(ref_pts), rstride, B, H, W,
                                                8, 8, 256, N.ptr(out), N.stream()), "lss_deform_attn_pts_fwd")
    return out


def deform_attn_bwd(value, offsets_logits, ref_pts, d_out, H, W):
    """Backward of `deform_attn_pts` (lss_deform_attn_bwd) -> d_value (B, H*W, 256), d_offsets_logits
    (B, H*W, 192), both fp32.  d_value is reduced in int64 fixed point: bit-reproducible, no float atomics."""
    B = value.shape[0]
    _f32c(value, "value", (B, H * W, 256))
    _f32c(offsets_logits, "offsets_logits", (B, H * W, 192))
    _f32c(d_out, "d_out", (B, H * W, 256))
    ref_pts, rstride = _ref_pts_arg(ref_pts, B, H * W)
    nbytes = N.lib().lss_deform_attn_bwd_workspace_bytes(B, H, W)
    ws = torch.empty((nbytes + 15) // 16, 2, dtype=torch.int64, device=value.device)
    d_value = torch.empty_like(value)
    d_ol = torch.empty_like(offsets_logits)
    with _timed("deform_attn_bwd"):
        N.check(N.lib().lss_deform_attn_bwd(N.ptr(value), N.ptr(offsets_logits), N.ptr(ref_pts), rstride, N.ptr(d_out),
                                            B, H, W, 8, 8, 256, N.ptr(ws), ws.numel() * 8, N.ptr(d_value), N.ptr(d_ol),
                                            N.stream()), "lss_deform_attn_bwd")
    return d_value, d_ol


def layernorm(x, gamma, beta, eps, out_dtype):
    """nn.LayerNorm over the last (256-wide) dim of contiguous fp32|bf16 rows."""
    if not x.is_contiguous() or x.dtype not in _DT:
        raise ValueError("x must be contiguous fp32/bf16")
    C = x.shape[-1]
    _f32c(gamma, "gamma", (C,))
    _f32c(beta, "beta", (C,))
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    with _timed("layernorm"):
        N.check(N.lib().lss_layernorm_fwd(N.ptr(x), _DT[x.dtype], N.ptr(gamma), N.ptr(beta), x.numel() // C, C,
                                          float(eps), N.ptr(y), _DT[out_dtype], N.stream()), "lss_layernorm_fwd")
    return y


def pack_conv_weight(w_oihw, dt):
    """OIHW fp32 -> the conv kernels' [tap][Cout][Cin] layout in `dt`."""
    Cout, Cin, KH, KW = w_oihw.shape
    _f32c(w_oihw, "conv weight")
    out = torch.empty(KH * KW, Cout, Cin, dtype=_TORCH_DT[dt], device=w_oihw.device)
    nbytes = N.lib().lss_conv2d_packed_weight_bytes(Cout, Cin, KH, KW, dt)
    assert nbytes == out.numel() * out.element_size()
    N.check(N.lib().lss_conv2d_pack_weights(N.ptr(w_oihw), Cout, Cin, KH, KW, dt, N.ptr(out), N.stream()),
            "lss_conv2d_pack_weights")
    return out


class RingWeight:
    """3x3 weights in the loader / consumer ring kernel's layout (csrc/conv_ring.hip): `data` is the flat bf16
    image, `Cout`, `Cin` the logical shape."""

    def __init__(self, data, Cout, Cin):
        self.data, self.Cout, self.Cin = data, Cout, Cin


class KsWeight(RingWeight):
    """3x3 weights in the layout of the K-split one-pass kernel (csrc/conv_ks.hip)."""


def conv_ks_ok(B, H, W, Cin, Cout):
    """Is this 3x3 / stride-1 / pad-1 bf16 conv a case for the K-split one-pass kernel (lss_conv2d_ks_ok)?"""
    return bool(N.lib().lss_conv2d_ks_ok(B, H, W, Cin, Cout))


def pack_conv_weight_ks(w_oihw, dgrad=False):
    """OIHW fp32 (3x3) -> KsWeight; dgrad=True: the weights of the layer's input-gradient conv (Cout -> Cin channels,
    transposed and tap-flipped), as the training units pack them."""
    Cout, Cin, KH, KW = w_oihw.shape
    _f32c(w_oihw, "conv weight")
    co, ci = (Cin, Cout) if dgrad else (Cout, Cin)   # channels of the conv the image is for
    nbytes = N.lib().lss_conv2d_ks_packed_weight_bytes(co, ci)
    if (KH, KW) != (3, 3) or nbytes == 0:
        raise ValueError("KS weights: 3x3, Cout %% 32 == 0, Cin in (64, 128, 256) (got %s%s)"
                         % (tuple(w_oihw.shape), ", dgrad" if dgrad else ""))
    out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w_oihw.device)
    fn = N.lib().lss_conv2d_pack_weights_ks_dgrad if dgrad else N.lib().lss_conv2d_pack_weights_ks
    N.check(fn(N.ptr(w_oihw), Cout, Cin, N.ptr(out), N.stream()), "lss_conv2d_pack_weights_ks")
    return KsWeight(out, co, ci)


def conv_ring_ok(B, H, W, Cx, C2, up, Cout, head_n=0):
    """Is this 3x3 / stride-1 / pad-1 bf16 conv a case for the ring kernel (lss_conv2d_ring_ok)?"""
    if os.environ.get("LSS_CONV_RING") == "0":
        return False
    return bool(N.lib().lss_conv2d_ring_ok(B, H, W, Cx, C2, up, Cout, head_n))


def pack_conv_weight_ring(w_oihw):
    """OIHW fp32 (3x3) -> RingWeight."""
    Cout, Cin, KH, KW = w_oihw.shape
    _f32c(w_oihw, "conv weight")
    nbytes = N.lib().lss_conv2d_ring_packed_weight_bytes(Cout, Cin)
    if (KH, KW) != (3, 3) or nbytes == 0:
        raise ValueError("ring weights: 3x3, Cout % 128 == 0, Cin % 32 == 0 (got %s)" % (tuple(w_oihw.shape),))
    out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w_oihw.device)
    N.check(N.lib().lss_conv2d_pack_weights_ring(N.ptr(w_oihw), Cout, Cin, N.ptr(out), N.stream()),
            "lss_conv2d_pack_weights_ring")
    return RingWeight(out, Cout, Cin)


def pack_conv_weight_ring_dgrad(w_oihw):
    """OIHW fp32 (3x3) -> RingWeight of the conv that maps dY (Cout channels) to dX (Cin channels)."""
    Cout, Cin, KH, KW = w_oihw.shape
    _f32c(w_oihw, "conv weight")
    nbytes = N.lib().lss_conv2d_ring_packed_weight_bytes(Cin, Cout)
    if (KH, KW) != (3, 3) or nbytes == 0:
        raise ValueError("ring dgrad weights: 3x3, Cin % 128 == 0, Cout % 32 == 0 (got %s)" % (tuple(w_oihw.shape),))
    out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w_oihw.device)
    N.check(N.lib().lss_conv2d_pack_weights_ring_dgrad(N.ptr(w_oihw), Cout, Cin, N.ptr(out), N.stream()),
            "lss_conv2d_pack_weights_ring_dgrad")
    return RingWeight(out, Cin, Cout)


# kind of a lss_conv_launch_t -> the entry lss_conv2d_sequence hands it to (named in error messages)
_CONV_ENTRIES = ("lss_conv2d_fwd", "lss_conv2d_s2_fwd", "lss_conv2d_head_fwd", "lss_conv2d_s2_dual_fwd",
                 "lss_conv2d_ks_s2_dual_fwd", "lss_conv2d_ks_stem_fwd")


def _conv_launch(kind, tag, tensors, dt=DT_BF16, **fields):
    """The one route from a conv wrapper to its kernel: one lss_conv_launch_t of `kind` from the pointer fields
    `tensors` (name -> GPU tensor or None) and the integer `fields`, handed to the recorder when one is set and run
    through lss_conv2d_sequence - the call a ConvPlan replays it with."""
    for name, t in tensors.items():
        if t is not None:
            if not t.is_cuda:
                raise N.LssNativeError("%s: expected a GPU tensor, got %s" % (name, t.device))
            fields[name] = t.data_ptr()
    c = N.ConvLaunch(kind=kind, dt=dt, **fields)
    if _recorder is not None:
        _recorder.add(c, [t for t in tensors.values() if t is not None])
    with _timed(tag):
        N.check(N.lib().lss_conv2d_sequence(ctypes.byref(c), 1, N.stream()), _CONV_ENTRIES[kind])


def _check_per_channel(n, **operands):
    """The optional per-channel fp32 operands of a conv epilogue: scale / shift (n = Cout), stats (n = 2 Cout)."""
    for name, t in operands.items():
        if t is not None:
            _f32c(t, name, (n,))


def conv2d_nhwc(x, w_packed, ksize, stride, pad, scale=None, shift=None, residual=None, relu=False,
                x2=None, up=1, stats=None, dt=DT_BF16, tag="conv2d_fwd", out_f32=False, head_major=False):
    """K8.  x (B,H,W,Cx) NHWC in `dt`; x2 (B,H*up,W*up,C2) optional skip tensor
    (conv input = cat([x2, upsample(x, up)])).  Returns y (B,Ho,Wo,Cout) in `dt`
    (fp32 with out_f32).  relu: False/True or an ACT_* code (ACT_GELU = erf GELU).
    head_major (1x1 bf16 convs): y is laid out (B, Cout/32, Ho*Wo, 32) and returned with that shape."""
    tdt = _TORCH_DT[dt]
    act = int(relu) | (OUT_F32 if (out_f32 and dt == DT_BF16) else 0) | (OUT_HEAD_MAJOR32 if head_major else 0)
    B, H, W, Cx = x.shape
    KH, KW = ksize
    if isinstance(w_packed, RingWeight):  # the ring / KS kernels' layouts (3x3 / s1 / p1 bf16 only; the C side checks)
        act |= W_KS if isinstance(w_packed, KsWeight) else W_RING
        taps, Cout, Cin, w_packed = 9, w_packed.Cout, w_packed.Cin, w_packed.data
    else:
        taps, Cout, Cin = w_packed.shape
    C2 = 0
    if x.dtype != tdt or not x.is_contiguous() or w_packed.dtype != tdt or not w_packed.is_contiguous():
        raise ValueError("conv operands must be contiguous %s" % tdt)
    if x2 is not None:
        if x2.dtype != tdt or not x2.is_contiguous() or tuple(x2.shape[:3]) != (B, H * up, W * up):
            raise ValueError("x2 must be contiguous %s of shape (B,H*up,W*up,C2)" % tdt)
        C2 = x2.shape[3]
    if taps != KH * KW or Cin != Cx + C2:
        raise ValueError("packed weight %s does not match Cin=%d taps=%d" % (tuple(w_packed.shape), Cx + C2, KH * KW))
    Ho = (H * up + 2 * pad - KH) // stride + 1
    Wo = (W * up + 2 * pad - KW) // stride + 1
    y = torch.empty(B, Ho, Wo, Cout, dtype=torch.float32 if out_f32 else tdt, device=x.device)
    _check_per_channel(Cout, scale=scale, shift=shift)
    _check_per_channel(2 * Cout, stats=stats)
    if residual is not None and (residual.dtype != tdt or tuple(residual.shape) != (B, Ho, Wo, Cout)
                                 or not residual.is_contiguous()):
        raise ValueError("residual must match the output")
    _conv_launch(0, tag, {"x": x, "x2": x2, "w": w_packed, "scale": scale, "shift": shift, "residual": residual, "y": y,
                          "stats": stats},
                 B=B, H=H, W=W, Cx=Cx, C2=C2, up=up, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad, relu=act, dt=dt)
    return y.view(B, Cout // 32, Ho * Wo, 32) if head_major else y


def pack_conv_weight_dgrad(w_oihw, dt):
    """OIHW fp32 -> [tap'][Cin][Cout] in dt: the weight of the conv that maps dY to dX
    (use with conv2d_nhwc(dy, w, (KH,KW), 1, KH-1-pad))."""
    Cout, Cin, KH, KW = w_oihw.shape
    _f32c(w_oihw, "conv weight")
    out = torch.empty(KH * KW, Cin, Cout, dtype=_TORCH_DT[dt], device=w_oihw.device)
    N.check(N.lib().lss_conv2d_pack_weights_dgrad(N.ptr(w_oihw), Cout, Cin, KH, KW, dt, N.ptr(out), N.stream()),
            "lss_conv2d_pack_weights_dgrad")
    return out


_wgrad_ws = {}


def conv3x3_wgrad(x, dy):
    """Weight gradient of a 3x3/s1/p1 conv.  x (B,H,W,Cin), dy (B,H,W,Cout) contiguous bf16 NHWC
    -> dW (Cout,Cin,3,3) fp32.  The workspace is cached per shape and device."""
    B, H, W, Cin = x.shape
    Cout = dy.shape[3]
    for t, nm in ((x, "x"), (dy, "dy")):
        if t.dtype != torch.bfloat16 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("%s must be a contiguous bf16 NHWC GPU tensor" % nm)
    if tuple(dy.shape[:3]) != (B, H, W):
        raise ValueError("dy %s does not match x %s" % (tuple(dy.shape), tuple(x.shape)))
    nbytes = N.lib().lss_conv2d_wgrad_workspace_bytes(B, H, W, Cin, Cout)
    ws = _cached_ws(_wgrad_ws, (B, H, W, Cin, Cout, str(x.device)), nbytes, x.device)
    dw = torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=x.device)
    with _timed("conv2d_wgrad"):
        N.check(N.lib().lss_conv2d_wgrad(N.ptr(x), N.ptr(dy), B, H, W, Cin, Cout, N.ptr(ws), nbytes, N.ptr(dw),
                                         N.stream()), "lss_conv2d_wgrad")
    return dw


def linear_wgrad_ok(T, Nout, K):
    """True when `linear_wgrad` accepts the shape (Nout % 64 == 0, K % 64 == 0, 64 <= Nout, K <= 1024, 1 <= T <= 2^22)."""
    return bool(N.lib().lss_linear_wgrad_ok(int(T), int(Nout), int(K)))


def linear_wgrad(x, dy, want_dw=True, want_db=True):
    """K11: weight and bias gradient of y = x W^T + b (lss_linear_wgrad).  x (T, K), dy (T, Nout) contiguous bf16 token
    rows -> (dw (Nout, K) fp32 | None, db (Nout) fp32 | None), bit-reproducible.  The workspace is cached per shape
    and device."""
    for t, nm in ((x, "x"), (dy, "dy")):
        if t.dim() != 2 or t.dtype != torch.bfloat16 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous 2-d bf16 tensor, got %s %s" % (nm, t.dtype, tuple(t.shape)))
    T, K = x.shape
    if dy.shape[0] != T:
        raise ValueError("dy %s does not match x %s" % (tuple(dy.shape), tuple(x.shape)))
    Nout = dy.shape[1]
    if not (want_dw or want_db):
        raise ValueError("linear_wgrad: nothing asked for")
    if not linear_wgrad_ok(T, Nout, K):
        raise ValueError("linear_wgrad needs N %% 64 == 0, K %% 64 == 0, 64 <= N, K <= 1024, 1 <= T <= 2^22 "
                         "(got T=%d, N=%d, K=%d)" % (T, Nout, K))
    if not (x.is_cuda and dy.is_cuda):
        raise ValueError("x and dy must be GPU tensors")
    nbytes = N.lib().lss_linear_wgrad_workspace_bytes(T, Nout, K)
    ws = _cached_ws(_wgrad_ws, ("linear", T, Nout, K, str(x.device)), nbytes, x.device)
    dw = torch.empty(Nout, K, dtype=torch.float32, device=x.device) if want_dw else None
    db = torch.empty(Nout, dtype=torch.float32, device=x.device) if want_db else None
    with _timed("linear_wgrad"):
        N.check(N.lib().lss_linear_wgrad(N.ptr(x), N.ptr(dy), T, Nout, K, N.ptr(ws), nbytes, N.ptr(dw), N.ptr(db),
                                         N.stream()), "lss_linear_wgrad")
    return dw, db


def _ln_bwd(fused, x, dy, gamma, eps, out_dtype, thr=0, scale=1.0, seed=None):
    """What `layernorm_bwd` (fused False: x in fp32 | bf16, dx in out_dtype) and `add_dropout_layernorm_bwd` (fused True:
    x = s fp32, ds fp32, da in out_dtype) share once their first operand is checked: the checks on dy, gamma, rows and
    devices, the workspace cached per row count and device, the (2, C) dgamma / dbeta buffer and the call.
    Returns (dx, da | None, dgamma, dbeta)."""
    name, xn, on = ("add_dropout_layernorm_bwd", "s", "da_dtype") if fused else ("layernorm_bwd", "x", "dx_dtype")
    if not dy.is_contiguous() or dy.dtype not in _DT:
        raise ValueError("dy must be contiguous fp32/bf16")
    if out_dtype not in _DT:
        raise ValueError("%s must be fp32 or bf16" % on)
    if tuple(dy.shape) != tuple(x.shape) or (not fused and x.numel() == 0):
        raise ValueError("dy %s does not match %s %s" % (tuple(dy.shape), xn, tuple(x.shape)))
    lib = N.lib()
    if fused:
        rows = _add_dropout_ln_rows(x, name)
    else:
        rows = x.numel() // x.shape[-1]
        if not lib.lss_layernorm_bwd_ok(rows, x.shape[-1]):
            raise ValueError("layernorm_bwd needs rows of 256 (got %s)" % (tuple(x.shape),))
    C = x.shape[-1]
    _f32c(gamma, "gamma", (C,))
    if not (x.is_cuda and dy.is_cuda):
        raise ValueError("%s and dy must be GPU tensors" % xn)
    nbytes = (lib.lss_add_dropout_ln_bwd_workspace_bytes if fused else lib.lss_layernorm_bwd_workspace_bytes)(rows)
    ws = _cached_ws(_wgrad_ws, ("add_dropout_ln" if fused else "layernorm", rows, str(x.device)), nbytes, x.device)
    dx = torch.empty(x.shape, dtype=torch.float32 if fused else out_dtype, device=x.device)
    da = torch.empty(x.shape, dtype=out_dtype, device=x.device) if fused else None
    dgb = torch.empty(2, C, dtype=torch.float32, device=x.device)
    with _timed(name):
        if fused:
            rc = lib.lss_add_dropout_ln_bwd(N.ptr(x), N.ptr(dy), _DT[dy.dtype], N.ptr(gamma), rows, C, float(eps), thr,
                                            scale, N.ptr(seed), N.ptr(ws), nbytes, N.ptr(dx), N.ptr(da), _DT[out_dtype],
                                            N.ptr(dgb[0]), N.ptr(dgb[1]), N.stream())
        else:
            rc = lib.lss_layernorm_bwd(N.ptr(x), _DT[x.dtype], N.ptr(dy), _DT[dy.dtype], N.ptr(gamma), rows, C,
                                       float(eps), N.ptr(ws), nbytes, N.ptr(dx), _DT[out_dtype], N.ptr(dgb[0]),
                                       N.ptr(dgb[1]), N.stream())
        N.check(rc, "lss_add_dropout_ln_bwd" if fused else "lss_layernorm_bwd")
    return dx, da, dgb[0], dgb[1]


def layernorm_bwd(x, dy, gamma, eps, dx_dtype):
    """K11: backward of `layernorm` (lss_layernorm_bwd).  x, dy contiguous fp32 | bf16 rows of 256, gamma (256) fp32 ->
    (dx like x in dx_dtype, dgamma (256), dbeta (256) fp32).  Mean and 1 / sigma are recomputed from x."""
    if not x.is_contiguous() or x.dtype not in _DT:
        raise ValueError("x must be contiguous fp32/bf16")
    dx, _, dgamma, dbeta = _ln_bwd(False, x, dy, gamma, eps, dx_dtype)
    return dx, dgamma, dbeta


def dropout_seed(device):
    """The 16-byte seed {key, stream} of one dropout site of the K12 kernels: ONE draw of two full-range int64 on the
    device from torch's generator of that device.  No host sync; reproducible after `torch.manual_seed`; a captured
    graph draws a fresh seed at every replay."""
    return torch.randint(-2 ** 63, 2 ** 63 - 1, (2,), dtype=torch.int64, device=device)


def dropout_threshold(p):
    """p -> (thr, scale) of the K12 mask (keep <=> 16-bit piece >= thr; thr = round(p * 65536), realised probability
    thr / 65536, scale = 1 / (1 - thr / 65536) as fp32), or None when p has no threshold in 0 .. 65535 (p < 0, p so
    close to 1 that everything would be dropped): such a p belongs to the torch composition."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        return None
    thr = int(round(p * 65536.0))
    if thr > 65535:
        return None
    return thr, 1.0 / (1.0 - thr / 65536.0)


def _mask_args(p, seed, device):
    """(thr, scale) of a K12 call; seed None = no dropout."""
    if seed is None:
        return 0, 1.0
    ts = dropout_threshold(p)
    if ts is None:
        raise ValueError("dropout p = %r has no 16-bit threshold" % (p,))
    if seed.dtype != torch.int64 or tuple(seed.shape) != (2,) or not seed.is_contiguous() or seed.device != device:
        raise ValueError("seed must be a contiguous int64 tensor of shape (2,) on the inputs' device")
    return ts


def _gelu_dropout_check(h, dy=None):
    for t, nm in ((h, "h"), (dy, "dy")):
        if t is not None and (t.dtype != torch.bfloat16 or not t.is_contiguous()):
            raise ValueError("%s must be a contiguous bf16 tensor, got %s" % (nm, t.dtype))
    if dy is not None and tuple(dy.shape) != tuple(h.shape):
        raise ValueError("dy %s does not match h %s" % (tuple(dy.shape), tuple(h.shape)))
    if not N.lib().lss_gelu_dropout_ok(h.numel()):
        raise ValueError("gelu_dropout needs a multiple of 8 elements, 8 <= n <= 2^32 (got %d)" % h.numel())
    if not (h.is_cuda and (dy is None or dy.is_cuda)):
        raise ValueError("h and dy must be GPU tensors")


def gelu_dropout(h, p=0.0, seed=None):
    """K12: dropout(gelu(h)) on the bf16 hidden in one pass (lss_gelu_dropout_fwd), exact-erf GELU in fp32.  The mask
    comes from `seed` (`dropout_seed`) and is never stored; seed None = no dropout."""
    thr, scale = _mask_args(p, seed, h.device)
    _gelu_dropout_check(h)
    y = torch.empty_like(h)
    with _timed("gelu_dropout"):
        N.check(N.lib().lss_gelu_dropout_fwd(N.ptr(h), h.numel(), thr, scale, N.ptr(seed), N.ptr(y), N.stream()),
                "lss_gelu_dropout_fwd")
    return y


def gelu_dropout_bwd(h, dy, p=0.0, seed=None):
    """K12: backward of `gelu_dropout` (lss_gelu_dropout_bwd): dh = dy * mask * gelu'(h), the mask recomputed."""
    thr, scale = _mask_args(p, seed, h.device)
    _gelu_dropout_check(h, dy)
    dh = torch.empty_like(h)
    with _timed("gelu_dropout_bwd"):
        N.check(N.lib().lss_gelu_dropout_bwd(N.ptr(h), N.ptr(dy), h.numel(), thr, scale, N.ptr(seed), N.ptr(dh), N.stream()),
                "lss_gelu_dropout_bwd")
    return dh


def _add_dropout_ln_rows(x, name):
    if x.dim() < 1 or x.numel() == 0 or not N.lib().lss_add_dropout_ln_ok(x.numel() // x.shape[-1], x.shape[-1]):
        raise ValueError("%s needs rows of 256, 1 <= rows <= 2^22 (got %s)" % (name, tuple(x.shape)))
    return x.numel() // x.shape[-1]


def add_dropout_layernorm(res, a, gamma, beta, eps, p=0.0, seed=None):
    """K12: s = res + dropout(a), y = LayerNorm(s) in one pass (lss_add_dropout_ln_fwd).  res, a contiguous fp32 | bf16
    rows of 256 of one shape -> (s, y), both fp32.  seed None = no dropout."""
    for t, nm in ((res, "res"), (a, "a")):
        if not t.is_contiguous() or t.dtype not in _DT:
            raise ValueError("%s must be contiguous fp32/bf16" % nm)
    if tuple(a.shape) != tuple(res.shape):
        raise ValueError("a %s does not match res %s" % (tuple(a.shape), tuple(res.shape)))
    rows = _add_dropout_ln_rows(res, "add_dropout_layernorm")
    C = res.shape[-1]
    _f32c(gamma, "gamma", (C,))
    _f32c(beta, "beta", (C,))
    thr, scale = _mask_args(p, seed, res.device)
    if not (res.is_cuda and a.is_cuda):
        raise ValueError("res and a must be GPU tensors")
    s = torch.empty(res.shape, dtype=torch.float32, device=res.device)
    y = torch.empty_like(s)
    with _timed("add_dropout_layernorm"):
        N.check(N.lib().lss_add_dropout_ln_fwd(N.ptr(res), _DT[res.dtype], N.ptr(a), _DT[a.dtype], rows, C, thr,
                                               scale, N.ptr(seed), N.ptr(gamma), N.ptr(beta), float(eps), N.ptr(s), N.ptr(y),
                                               N.stream()), "lss_add_dropout_ln_fwd")
    return s, y


def add_dropout_layernorm_bwd(s, dy, gamma, eps, da_dtype, p=0.0, seed=None):
    """K12: backward of `add_dropout_layernorm` (lss_add_dropout_ln_bwd).  s (the saved fp32 sum), dy fp32 | bf16 ->
    (ds fp32 = the gradient of res, da = ds * mask in da_dtype, dgamma, dbeta fp32).  The workspace is cached per row
    count and device, as `layernorm_bwd`'s."""
    if not s.is_contiguous() or s.dtype != torch.float32:
        raise ValueError("s must be contiguous fp32")
    return _ln_bwd(True, s, dy, gamma, eps, da_dtype, *_mask_args(p, seed, s.device), seed)


def pack_conv_weight_s2_dgrad(w_oihw, pad):
    """OIHW fp32 of a stride-2 K x K conv -> (KT*KT, 4*Cin, Cout) bf16: the weight of the stride-1 conv that maps dY to
    the four phase planes of dX (lss_conv2d_pack_weights_s2_dgrad).  Returns (packed, KT)."""
    Cout, Cin, K, _ = w_oihw.shape
    _f32c(w_oihw, "conv weight")
    KT = N.lib().lss_conv2d_s2_dgrad_taps(K, pad)
    if KT == 0:
        raise ValueError("stride-2 data gradient: K / pad in (1, 0), (3, 1), (7, 3)")
    out = torch.empty(KT * KT, 4 * Cin, Cout, dtype=torch.bfloat16, device=w_oihw.device)
    N.check(N.lib().lss_conv2d_pack_weights_s2_dgrad(N.ptr(w_oihw), Cout, Cin, K, pad, N.ptr(out), N.stream()),
            "lss_conv2d_pack_weights_s2_dgrad")
    return out, KT


def conv4x4_wgrad(xs, dy):
    """Weight gradient of the 4x4-tap stride-1 conv with taps (dy, dx) in {-2 .. 1}^2 (a 7x7 / 2 / pad-3 conv over
    phase planes): xs (B,H,W,Cin), dy (B,H,W,Cout) contiguous bf16 NHWC -> (Cout, Cin, 4, 4) fp32, tap [dy + 2][dx + 2]."""
    B, H, W, Cin = xs.shape
    Cout = dy.shape[3]
    for t, nm in ((xs, "xs"), (dy, "dy")):
        if t.dtype != torch.bfloat16 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("%s must be a contiguous bf16 NHWC GPU tensor" % nm)
    if tuple(dy.shape[:3]) != (B, H, W):
        raise ValueError("dy %s does not match xs %s" % (tuple(dy.shape), tuple(xs.shape)))
    nbytes = N.lib().lss_conv2d_wgrad4x4_workspace_bytes(B, H, W, Cin, Cout)
    if nbytes == 0:
        raise ValueError("conv4x4_wgrad: channel counts must be multiples of 64 and 8 <= W <= 224")
    ws = _cached_ws(_wgrad_ws, ("4x4", B, H, W, Cin, Cout, str(xs.device)), nbytes, xs.device)
    dw = torch.empty(Cout, Cin, 4, 4, dtype=torch.float32, device=xs.device)
    with _timed("conv2d_wgrad"):
        N.check(N.lib().lss_conv2d_wgrad4x4(N.ptr(xs), N.ptr(dy), B, H, W, Cin, Cout, N.ptr(ws), nbytes, N.ptr(dw),
                                            N.stream()), "lss_conv2d_wgrad4x4")
    return dw


def upsample_cat_nhwc(x, x2, up):
    """[x2 | bilinear_align_corners(x, up)] as a contiguous bf16 (B, H*up, W*up, C2+Cx) tensor."""
    B, H, W, Cx = x.shape
    C2 = 0 if x2 is None else x2.shape[3]
    for t in (x, x2):
        if t is not None and (t.dtype != torch.bfloat16 or not t.is_contiguous()):
            raise ValueError("upsample_cat_nhwc operands must be contiguous bf16 NHWC")
    if x2 is not None and tuple(x2.shape[:3]) != (B, H * up, W * up):
        raise ValueError("x2 %s does not match x %s upsampled x%d" % (tuple(x2.shape), tuple(x.shape), up))
    out = torch.empty(B, H * up, W * up, C2 + Cx, dtype=torch.bfloat16, device=x.device)
    with _timed("upsample_cat"):
        N.check(N.lib().lss_upsample_cat_nhwc(N.ptr(x), N.ptr(x2), B, H, W, Cx, C2, up, N.ptr(out), N.stream()),
                "lss_upsample_cat_nhwc")
    return out


def upsample_bwd_nhwc(g, c_off, Cx, up):
    """Adjoint of the bilinear (align_corners) x`up` upsample applied to channels [c_off, c_off+Cx)
    of g (B, H*up, W*up, Ct) bf16 -> (B, H, W, Cx) bf16."""
    B, Hh, Wh, Ct = g.shape
    if g.dtype != torch.bfloat16 or not g.is_contiguous() or Hh % up or Wh % up:
        raise ValueError("g must be contiguous bf16 NHWC with sizes divisible by the scale")
    dx = torch.empty(B, Hh // up, Wh // up, Cx, dtype=torch.bfloat16, device=g.device)
    with _timed("upsample_bwd"):
        N.check(N.lib().lss_upsample_bwd_nhwc(N.ptr(g), B, Hh // up, Wh // up, Cx, Ct, c_off, up, N.ptr(dx),
                                              N.stream()), "lss_upsample_bwd_nhwc")
    return dx


_bn_ws = {}


def _bn_workspace(M, C, device):
    key = (M, C, str(device))
    ws = _bn_ws.get(key)
    if ws is None:
        nbytes = N.lib().lss_bn_train_workspace_bytes(M, C)
        if nbytes == 0:
            raise ValueError("BatchNorm over %d rows x %d channels is outside the kernels' range" % (M, C))
        ws = _bn_ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def bn_train_fwd(z, gamma, beta, running_mean, running_var, momentum, eps, relu, residual=None):
    """Training-mode BatchNorm (+residual, +ReLU) on contiguous bf16 NHWC z (..., C).
    Returns y (bf16, like z), save_mean, save_invstd (fp32); running stats updated in place."""
    C = z.shape[-1]
    M = z.numel() // C
    for t, nm in ((z, "z"), (residual, "residual")):
        if t is not None and (t.dtype != torch.bfloat16 or not t.is_contiguous() or tuple(t.shape) != tuple(z.shape)):
            raise ValueError("%s must be contiguous bf16 shaped like z" % nm)
    _f32c(gamma, "gamma", (C,))
    _f32c(beta, "beta", (C,))
    if running_mean is not None:
        _f32c(running_mean, "running_mean", (C,))
        _f32c(running_var, "running_var", (C,))
    y = torch.empty_like(z)
    mean = torch.empty(C, dtype=torch.float32, device=z.device)
    invstd = torch.empty(C, dtype=torch.float32, device=z.device)
    with _timed("bn_train_fwd"):
        N.check(N.lib().lss_bn_train_fwd(N.ptr(z), N.ptr(residual), M, C, N.ptr(gamma), N.ptr(beta), N.ptr(running_mean),
                                         N.ptr(running_var), float(momentum), float(eps), 1 if relu else 0,
                                         N.ptr(_bn_workspace(M, C, z.device)), N.ptr(y), N.ptr(mean), N.ptr(invstd),
                                         N.stream()), "lss_bn_train_fwd")
    return y, mean, invstd


def bn_train_bwd(dy, y, z, gamma, mean, invstd, relu, want_dres):
    """Backward of bn_train_fwd: returns dz (bf16), dres (bf16 or None), dgamma, dbeta (fp32)."""
    C = z.shape[-1]
    M = z.numel() // C
    for t, nm in ((dy, "dy"), (z, "z"), (y, "y")):
        if t is not None and (t.dtype != torch.bfloat16 or not t.is_contiguous() or tuple(t.shape) != tuple(z.shape)):
            raise ValueError("%s must be contiguous bf16 shaped like z" % nm)
    dz = torch.empty_like(z)
    dres = torch.empty_like(z) if want_dres else None
    dgamma = torch.empty(C, dtype=torch.float32, device=z.device)
    dbeta = torch.empty(C, dtype=torch.float32, device=z.device)
    with _timed("bn_train_bwd"):
        N.check(N.lib().lss_bn_train_bwd(N.ptr(dy), N.ptr(y), N.ptr(z), M, C, N.ptr(gamma), N.ptr(mean), N.ptr(invstd),
                                         1 if relu else 0, N.ptr(_bn_workspace(M, C, z.device)), N.ptr(dz), N.ptr(dres),
                                         N.ptr(dgamma), N.ptr(dbeta), N.stream()), "lss_bn_train_bwd")
    return dz, dres, dgamma, dbeta


def bn_partial_sums(z, mode, dy=None, y=None, mean=None, invstd=None, relu=False):
    """(2, C) fp32 per-channel sums of this rank's rows: mode 0 = (sum z, sum z^2); mode 1 = (sum g, sum g*xhat)."""
    C = z.shape[-1]
    M = z.numel() // C
    sums = torch.empty(2, C, dtype=torch.float32, device=z.device)
    N.check(N.lib().lss_bn_partial_sums(N.ptr(z), N.ptr(dy), N.ptr(y), N.ptr(mean), N.ptr(invstd), M, C,
                                        1 if relu else 0, mode, N.ptr(_bn_workspace(M, C, z.device)), N.ptr(sums),
                                        N.stream()), "lss_bn_partial_sums")
    return sums


def bn_train_fwd_from_sums(z, sums, m_total, gamma, beta, running_mean, running_var, momentum, eps, relu, residual=None):
    C = z.shape[-1]
    M = z.numel() // C
    y = torch.empty_like(z)
    mean = torch.empty(C, dtype=torch.float32, device=z.device)
    invstd = torch.empty(C, dtype=torch.float32, device=z.device)
    N.check(N.lib().lss_bn_train_fwd_from_sums(N.ptr(z), N.ptr(residual), M, C, N.ptr(sums), int(m_total), N.ptr(gamma),
                                               N.ptr(beta), N.ptr(running_mean), N.ptr(running_var), float(momentum),
                                               float(eps), 1 if relu else 0, N.ptr(_bn_workspace(M, C, z.device)),
                                               N.ptr(y), N.ptr(mean), N.ptr(invstd), N.stream()),
            "lss_bn_train_fwd_from_sums")
    return y, mean, invstd


def bn_train_bwd_from_sums(dy, y, z, sums, m_total, gamma, mean, invstd, relu, want_dres):
    C = z.shape[-1]
    M = z.numel() // C
    dz = torch.empty_like(z)
    dres = torch.empty_like(z) if want_dres else None
    scratch = torch.empty(2, C, dtype=torch.float32, device=z.device)  # the global dgamma / dbeta (unused by DP callers)
    N.check(N.lib().lss_bn_train_bwd_from_sums(N.ptr(dy), N.ptr(y), N.ptr(z), M, C, N.ptr(sums), int(m_total),
                                               N.ptr(gamma), N.ptr(mean), N.ptr(invstd), 1 if relu else 0,
                                               N.ptr(_bn_workspace(M, C, z.device)), N.ptr(dz), N.ptr(dres),
                                               scratch.data_ptr(), scratch.data_ptr() + 4 * C, N.stream()),
            "lss_bn_train_bwd_from_sums")
    return dz, dres


def _p(t):
    return None if t is None else t.data_ptr()


class _GatherJob(ctypes.Structure):
    _fields_ = [("src", ctypes.c_void_p), ("idx", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("n", ctypes.c_longlong)]


class WeightPrepack:
    """Every packed weight image of a training step in ONE launch (csrc/layout.hip: lss_gather_pack).

    The weights change every step, so every conv unit packs its bf16 image(s) - tile / ring / K-split / phase-plane
    layout, forward and input-gradient form - on every call: 36 small launches per step of the benched model.  A packed
    image is a permutation of the layer's fp32 weights plus zeros, so it can be produced by a table-driven gather that
    knows nothing about layouts.  A unit REGISTERS its image the first time it packs one (eager warm-up steps): the
    table comes from pushing the three byte planes of the element numbers 1..n through the unit's own pack routine
    (values <= 255 are exact in bf16), and is checked once against that routine on the real weights.  From then on
    `run(params)` - called by dp.train_step* at the top of a step with the step's trainable tensors - fills their
    registered images with one launch (images of tensors that are gone are dropped, not read), and the units find
    theirs through `lookup` instead of packing; `invalidate()` after the optimizer step makes them pack
    themselves again unless another `run()` comes first, so a caller with its own loop is never handed a stale image.
    Keys are (weight address, shape, kind): whatever lives at that address is what gets packed.  LSS_PREPACK=0 disables."""

    def __init__(self):
        self.jobs = {}
        self._table = None
        self._tls = threading.local()   # `fresh` belongs to the thread that ran the step's `run()`

    @property
    def fresh(self):
        return getattr(self._tls, "fresh", False)

    @fresh.setter
    def fresh(self, v):
        self._tls.fresh = bool(v)

    @staticmethod
    def enabled():
        return os.environ.get("LSS_PREPACK", "1") != "0"

    @staticmethod
    def _key(w, kind):
        return (w.data_ptr(), tuple(w.shape), str(w.device)) + tuple(kind)

    def lookup(self, w, kind):
        if not self.fresh:
            return None
        j = self.jobs.get(self._key(w, kind))
        return None if j is None else j[2]

    def register(self, w, kind, pack_fn):
        """pack_fn(fp32 tensor shaped like w) -> the bf16 image (any shape); no-op while a stream capture is active."""
        if not self.enabled() or not w.is_cuda or w.dtype != torch.float32 or not w.is_contiguous():
            return
        if torch.cuda.is_current_stream_capturing() or w.numel() >= (1 << 24):
            return
        key = self._key(w, kind)
        if key in self.jobs:
            return
        n = w.numel()
        num = torch.arange(1, n + 1, device=w.device, dtype=torch.int64).view(w.shape)
        idx = None
        for b in range(3):
            img = pack_fn(((num >> (8 * b)) & 255).float())
            v = img.reshape(-1).float().to(torch.int64) << (8 * b)
            idx = v if idx is None else idx | v
        ref = pack_fn(w.detach())
        dst = torch.empty_like(ref)
        got = torch.where(idx > 0, w.detach().reshape(-1)[(idx - 1).clamp(min=0)], torch.zeros((), device=w.device))
        if not torch.equal(got.to(torch.bfloat16), ref.reshape(-1)):
            raise N.LssNativeError("WeightPrepack: the image of kind %s is not a permutation of its weights" % (kind,))
        self.jobs[key] = (w.data_ptr(), idx.to(torch.int32).contiguous(), dst)
        self._table = None

    def run(self, params):
        """Fill the registered images of `params` (the step's trainable tensors) from their current values: one launch
        per 96 images.  Images registered for tensors that are not among `params` any more - a model that has been
        deleted: its memory may be unmapped by now - are dropped, never read."""
        if not self.jobs or not self.enabled():
            return
        live = {p.data_ptr() for p in params}
        if any(j[0] not in live for j in self.jobs.values()):
            self.jobs = {k: j for k, j in self.jobs.items() if j[0] in live}
            self._table = None
            if not self.jobs:
                return
        if self._table is None:
            tab = (_GatherJob * len(self.jobs))()
            for i, (src, idx, dst) in enumerate(self.jobs.values()):
                tab[i].src, tab[i].idx, tab[i].dst, tab[i].n = src, idx.data_ptr(), dst.data_ptr(), idx.numel()
            self._table = tab
        N.check(N.lib().lss_gather_pack(ctypes.cast(self._table, ctypes.c_void_p), len(self.jobs), N.stream()),
                "lss_gather_pack")
        self.fresh = True

    def invalidate(self):
        self.fresh = False

    def clear(self):
        """Forget every registered image (the units pack and register again on their next call)."""
        self.jobs = {}
        self._table = None
        self.fresh = False


prepack = WeightPrepack()


def prepacked(w, kind, pack_fn):
    """The bf16 image of weights `w` a unit needs: the step's pre-packed one when `prepack.run()` has filled it,
    else packed now (and registered for the next steps)."""
    pk = prepack.lookup(w, kind)
    if pk is not None:
        return pk
    out = pack_fn(w)
    prepack.register(w, kind, pack_fn)
    return out


def _unit_pack_fn(B, H, W, Cx, C2, up, Cout, dgrad):
    def fn(w):
        out = torch.empty(9 * Cout * (Cx + C2), dtype=torch.bfloat16, device=w.device)
        N.check(N.lib().lss_conv_bn_act_train_pack(w.data_ptr(), B, H, W, Cx, C2, up, Cout, dgrad, out.data_ptr(),
                                                   N.stream()), "lss_conv_bn_act_train_pack")
        return out
    return fn


def conv_bn_act_train_fwd(x1n, x2n, weight, gamma, beta, resn, running_mean, running_var, momentum, eps, relu, up):
    """One host call: conv3x3 (fused upsample/concat input) -> BN(train) -> (+res) -> ReLU.  Operands are
    trusted (contiguous bf16 NHWC activations, fp32 parameters): the caller is modules._ConvBNActFn.
    Returns z, y (bf16 NHWC), save_mean, save_invstd."""
    B, H, W, Cx = x1n.shape
    C2 = 0 if x2n is None else x2n.shape[3]
    Cout = weight.shape[0]
    dev = x1n.device
    z = torch.empty(B, H * up, W * up, Cout, dtype=torch.bfloat16, device=dev)
    y = torch.empty_like(z)
    kind = ("unit", 0, B, H, W, Cx, C2, up)
    wp = prepack.lookup(weight, kind)          # filled by prepack.run() at the top of the step, or ...
    wsrc = None
    if wp is None:                             # ... packed inside the call (and registered for the next steps)
        wp = torch.empty(9 * Cout * (Cx + C2), dtype=torch.bfloat16, device=dev)
        wsrc = weight
        prepack.register(weight, kind, _unit_pack_fn(B, H, W, Cx, C2, up, Cout, 0))
    stat = torch.empty(2, Cout, dtype=torch.float32, device=dev)
    ws = _bn_workspace(B * H * up * W * up, Cout, dev)
    with _timed("conv_bn_act_train_fwd"):
        N.check(N.lib().lss_conv_bn_act_train_fwd(
            x1n.data_ptr(), _p(x2n), _p(wsrc), gamma.data_ptr(), beta.data_ptr(), _p(resn), _p(running_mean),
            _p(running_var), wp.data_ptr(), z.data_ptr(), y.data_ptr(), stat.data_ptr(), stat.data_ptr() + 4 * Cout,
            ws.data_ptr(), B, H, W, Cx, C2, up, Cout, momentum, eps, 1 if relu else 0, N.stream()),
            "lss_conv_bn_act_train_fwd")
    return z, y, stat


def conv_bn_act_train_bwd(gyn, y, z, x1n, x2n, weight, gamma, stat, relu, up, want_res, want_x1, want_x2, want_w):
    """Backward of conv_bn_act_train_fwd in one host call.  Returns (g1, g2, gw, dgamma, dbeta, dres)."""
    B, H, W, Cx = x1n.shape
    C2 = 0 if x2n is None else x2n.shape[3]
    Cout, Ct = weight.shape[0], Cx + C2
    Hh, Wh = H * up, W * up
    dev = x1n.device
    dz = torch.empty_like(z)
    dres = torch.empty_like(z) if want_res else None
    dgb = torch.empty(2, Cout, dtype=torch.float32, device=dev)
    plain = up == 1 and C2 == 0
    gcat = g1 = xcat = gw = wd = wws = wsrc = None   # wsrc: the fp32 weights, when the call has to pack the dgrad image
    nws = 0
    if want_x1 or want_x2:
        gcat = torch.empty(B, Hh, Wh, Ct, dtype=torch.bfloat16, device=dev)
        kind = ("unit", 1, B, H, W, Cx, C2, up)
        wd = prepack.lookup(weight, kind)
        if wd is None:
            wd = torch.empty(9 * Cout * Ct, dtype=torch.bfloat16, device=dev)
            wsrc = weight
            prepack.register(weight, kind, _unit_pack_fn(B, H, W, Cx, C2, up, Cout, 1))
        if want_x1 and not plain:
            g1 = torch.empty(B, H, W, Cx, dtype=torch.bfloat16, device=dev)
    if want_w:
        gw = torch.empty(Cout, Ct, 3, 3, dtype=torch.float32, device=dev)
        if not plain:
            xcat = torch.empty(B, Hh, Wh, Ct, dtype=torch.bfloat16, device=dev)
        nws = N.lib().lss_conv2d_wgrad_workspace_bytes(B, Hh, Wh, Ct, Cout)
        wws = _cached_ws(_wgrad_ws, (B, Hh, Wh, Ct, Cout, str(dev)), nws, dev)
    ws = _bn_workspace(B * Hh * Wh, Cout, dev)
    with _timed("conv_bn_act_train_bwd"):
        N.check(N.lib().lss_conv_bn_act_train_bwd(
            gyn.data_ptr(), y.data_ptr(), z.data_ptr(), x1n.data_ptr(), _p(x2n), _p(wsrc), gamma.data_ptr(),
            stat.data_ptr(), stat.data_ptr() + 4 * Cout, ws.data_ptr(), _p(wws), nws, _p(wd), dz.data_ptr(), _p(dres),
            dgb.data_ptr(), dgb.data_ptr() + 4 * Cout, _p(gcat), _p(g1), _p(xcat), _p(gw), B, H, W, Cx, C2, up, Cout,
            1 if relu else 0, N.stream()), "lss_conv_bn_act_train_bwd")
    if want_x1 and plain:
        g1 = gcat
    g2 = gcat[..., :C2] if (want_x2 and C2 > 0) else None
    return g1, g2, gw, dgb[0], dgb[1], dres


def weighted_ce_fwd(logits, target, weight):
    """loss (1-element fp32 tensor) and the saved sums for weighted_ce_bwd.  logits (B,C,...) fp32
    contiguous, target (B,...) int64 contiguous, weight (C) fp32."""
    B, C = logits.shape[:2]
    _f32c(logits, "logits")
    _f32c(weight, "weight", (C,))
    if target.dtype != torch.int64 or not target.is_contiguous() or target.numel() * C != logits.numel():
        raise ValueError("target must be contiguous int64 of shape (B, ...) matching the logits")
    HW = logits.numel() // (B * C)
    ws = torch.empty(512 + 3, dtype=torch.float32, device=logits.device)
    with _timed("weighted_ce_fwd"):
        N.check(N.lib().lss_weighted_ce_fwd(N.ptr(logits), N.ptr(target), N.ptr(weight), B, C, HW, ws.data_ptr(),
                                            ws.data_ptr() + 4 * 512, ws.data_ptr() + 4 * 514, N.stream()),
                "lss_weighted_ce_fwd")
    return ws[514:515].view(()), ws[512:514]


def weighted_ce_bwd(logits, target, weight, sums, grad_loss):
    B, C = logits.shape[:2]
    HW = logits.numel() // (B * C)
    g = torch.empty_like(logits)
    gl = grad_loss.reshape(1).float().contiguous()
    with _timed("weighted_ce_bwd"):
        N.check(N.lib().lss_weighted_ce_bwd(N.ptr(logits), N.ptr(target), N.ptr(weight), B, C, HW, N.ptr(sums),
                                            N.ptr(gl), N.ptr(g), N.stream()), "lss_weighted_ce_bwd")
    return g


_head_ce_ws = {}


def _head_ce_workspace(K, device):
    key = (K, str(device))
    ws = _head_ce_ws.get(key)
    if ws is None:
        nbytes = N.lib().lss_head_ce_workspace_bytes(K)
        if nbytes == 0:
            raise ValueError("fused head + cross-entropy supports 4 or 8 classes")
        ws = _head_ce_ws[key] = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    return ws


def _head_shape(head_w):
    K, Cin = head_w.shape
    if Cin not in (64, 128) or K not in (4, 8):
        raise ValueError("the head kernels take 64 or 128 input channels and 4 or 8 classes, got head_w %s"
                         % (tuple(head_w.shape),))
    return K, Cin


def head_ce_fwd(y, head_w, head_b, target, class_w):
    """Fused 1x1 head + weighted cross-entropy.  y (..., Cin) contiguous bf16 NHWC rows, Cin = 64 or 128; head_w
    (K, Cin) fp32, K = 4 or 8; head_b (K); target int64 with y's leading shape; class_w (K).  Returns (loss 0-d
    tensor, sums (2,))."""
    K, Cin = _head_shape(head_w)
    if y.dtype != torch.bfloat16 or not y.is_contiguous() or y.shape[-1] != Cin:
        raise ValueError("y must be contiguous bf16 rows of %d channels" % Cin)
    _f32c(head_w, "head_w", (K, Cin))
    _f32c(head_b, "head_b", (K,))
    _f32c(class_w, "class_w", (K,))
    M = y.numel() // Cin
    if target.dtype != torch.int64 or not target.is_contiguous() or target.numel() != M or not target.is_cuda:
        raise ValueError("target must be a contiguous int64 GPU tensor with one entry per pixel")
    out = torch.empty(3, dtype=torch.float32, device=y.device)
    with _timed("head_ce_fwd"):
        N.check(N.lib().lss_head_ce_fwd(N.ptr(y), N.ptr(head_w), N.ptr(head_b), N.ptr(target), N.ptr(class_w), M, Cin, K,
                                        N.ptr(_head_ce_workspace(K, y.device)), out.data_ptr(), out.data_ptr() + 8,
                                        N.stream()), "lss_head_ce_fwd")
    return out[2].view(()), out[:2]


def head_ce_bwd(y, head_w, head_b, target, class_w, sums, grad_loss):
    """Backward of head_ce_fwd: returns (dy bf16 like y, d_head_w (K, Cin) fp32, d_head_b (K) fp32)."""
    K, Cin = _head_shape(head_w)
    M = y.numel() // Cin
    dy = torch.empty_like(y)
    dw = torch.empty(K, Cin, dtype=torch.float32, device=y.device)
    db = torch.empty(K, dtype=torch.float32, device=y.device)
    gl = grad_loss.reshape(1).float().contiguous()
    with _timed("head_ce_bwd"):
        N.check(N.lib().lss_head_ce_bwd(N.ptr(y), N.ptr(head_w), N.ptr(head_b), N.ptr(target), N.ptr(class_w), M, Cin, K,
                                        N.ptr(sums), N.ptr(gl), N.ptr(_head_ce_workspace(K, y.device)), N.ptr(dy),
                                        N.ptr(dw), N.ptr(db), N.stream()), "lss_head_ce_bwd")
    return dy, dw, db


def head1x1_fwd(y, head_w, head_b):
    """The 1x1 head alone: y (B, H, W, Cin) contiguous bf16, Cin = 64 or 128 -> logits (B, K, H, W) fp32 NCHW, K = 4 or
    8 (lss_head1x1_fwd)."""
    K, Cin = _head_shape(head_w)
    if y.dtype != torch.bfloat16 or not y.is_contiguous() or y.dim() != 4 or y.shape[-1] != Cin:
        raise ValueError("y must be a contiguous (B, H, W, %d) bf16 tensor" % Cin)
    _f32c(head_w, "head_w", (K, Cin))
    _f32c(head_b, "head_b", (K,))
    B, H, W, _ = y.shape
    out = torch.empty(B, K, H, W, dtype=torch.float32, device=y.device)
    with _timed("head1x1_fwd"):
        N.check(N.lib().lss_head1x1_fwd(N.ptr(y), N.ptr(head_w), N.ptr(head_b), B * H * W, H * W, Cin, K, N.ptr(out),
                                        N.stream()), "lss_head1x1_fwd")
    return out


def head1x1_bwd(y, head_w, head_b, grad_logits):
    """Backward of head1x1_fwd: grad_logits (B, K, H, W) fp32 contiguous -> (dy bf16 like y, d_head_w (K, Cin), d_head_b (K))."""
    K, Cin = _head_shape(head_w)
    B, H, W, _ = y.shape
    _f32c(grad_logits, "grad_logits", (B, K, H, W))
    dy = torch.empty_like(y)
    dw = torch.empty(K, Cin, dtype=torch.float32, device=y.device)
    db = torch.empty(K, dtype=torch.float32, device=y.device)
    with _timed("head1x1_bwd"):
        N.check(N.lib().lss_head1x1_bwd(N.ptr(y), N.ptr(head_w), N.ptr(head_b), N.ptr(grad_logits), B * H * W, H * W, Cin,
                                        K, N.ptr(_head_ce_workspace(K, y.device)), N.ptr(dy), N.ptr(dw), N.ptr(db),
                                        N.stream()), "lss_head1x1_bwd")
    return dy, dw, db


_seg_eval_ws = {}
SEG_EVAL_MAXC = 16
def _seg_eval_workspace(C, device):
    key = (C, str(device))
    ws = _seg_eval_ws.get(key)
    if ws is None:
        nbytes = N.lib().lss_seg_eval_workspace_bytes(C)
        if nbytes == 0:
            raise ValueError("the fused confusion-matrix pass supports 1..%d classes (got %d)" % (SEG_EVAL_MAXC, C))
        ws = _seg_eval_ws[key] = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
    return ws


def _seg_eval_counter(t, name, numel, dtype=torch.int64):
    if t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or t.numel() != numel:
        raise ValueError("%s must be a contiguous %s GPU tensor of %d elements" % (name, dtype, numel))
    return t


def seg_eval_update(logits, target, confmat, class_weight=None, loss_acc=None, invalid=None):
    """One pass over the segmentation logits of a batch (csrc/metrics.hip): `confmat` (C, C) int64 += the counts of
    (target, first maximal class) over the pixels whose target lies in [0, C); with `class_weight` (C) fp32 also the
    batch's weighted cross-entropy, returned as a 0-d fp32 tensor, and `loss_acc` (1 double) += loss * B.  logits
    (B, C, ...) contiguous fp32 or bf16, target (B, ...) contiguous int64.  Two launches, no host synchronisation.
    `invalid` (1 int64) is only checked: an argmax is always a class, so this form never adds to it."""
    if logits.dtype not in _DT or not logits.is_cuda or not logits.is_contiguous() or logits.dim() < 2:
        raise ValueError("logits must be a contiguous fp32 or bf16 GPU tensor of shape (B, C, ...)")
    B, C = logits.shape[:2]
    if not 1 <= C <= SEG_EVAL_MAXC or logits.numel() == 0:
        raise ValueError("logits need 1..%d classes and at least one pixel (got shape %s)"
                         % (SEG_EVAL_MAXC, tuple(logits.shape)))
    HW = logits.numel() // (B * C)
    if B * HW >= 2 ** 31:
        raise ValueError("B * H * W must stay below 2^31")
    if (target.dtype != torch.int64 or not target.is_cuda or not target.is_contiguous() or target.numel() != B * HW
            or target.shape[0] != B):
        raise ValueError("target must be a contiguous int64 GPU tensor of shape (B, ...) matching the logits")
    _seg_eval_counter(confmat, "confmat", C * C)
    if invalid is not None:
        _seg_eval_counter(invalid, "invalid", 1)
    loss = None
    if class_weight is not None:
        _f32c(class_weight, "class_weight", (C,))
        if loss_acc is not None:
            _seg_eval_counter(loss_acc, "loss_acc", 1, torch.float64)
        loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    elif loss_acc is not None:
        raise ValueError("loss_acc needs class_weight")
    ws = _seg_eval_workspace(C, logits.device)
    with _timed("seg_eval_update"):
        N.check(N.lib().lss_seg_eval_update(N.ptr(logits), _DT[logits.dtype], N.ptr(target), N.ptr(class_weight),
                                            B, C, HW, N.ptr(ws), ws.numel() * 4, N.ptr(confmat), N.ptr(loss),
                                            N.ptr(loss_acc), N.stream()), "lss_seg_eval_update")
    return None if loss is None else loss.view(())


def seg_eval_update_labels(pred, target, confmat, invalid):
    """`confmat` (C, C) int64 += the counts of (target, pred) over the elements whose target lies in [0, C); pred and
    target contiguous int64 GPU tensors of one size.  A pred outside [0, C) on a counted target adds 1 to `invalid`
    (1 int64) instead of the matrix.  Two launches, no host synchronisation."""
    C = confmat.shape[0] if confmat.dim() == 2 else 0
    if not 1 <= C <= SEG_EVAL_MAXC:
        raise ValueError("confmat must be (C, C) with 1..%d classes" % SEG_EVAL_MAXC)
    _seg_eval_counter(confmat, "confmat", C * C)
    _seg_eval_counter(invalid, "invalid", 1)
    n = pred.numel()
    if not 0 < n < 2 ** 31:
        raise ValueError("pred needs 1..2^31-1 elements")
    _seg_eval_counter(pred, "pred", n)
    _seg_eval_counter(target, "target", n)
    ws = _seg_eval_workspace(C, pred.device)
    with _timed("seg_eval_update"):
        N.check(N.lib().lss_seg_eval_update_labels(N.ptr(pred), N.ptr(target), n, C, N.ptr(ws), ws.numel() * 4,
                                                   N.ptr(confmat), N.ptr(invalid), N.stream()),
                "lss_seg_eval_update_labels")


def pack_conv_weight_s2d(w_oihw, pad):
    """OIHW fp32 of a stride-2 k x k conv -> bf16 [tap'][Cout][4*Cin] for conv2d_s2_nhwc."""
    Cout, Cin, K, K2 = w_oihw.shape
    _f32c(w_oihw, "conv weight")
    nbytes = N.lib().lss_conv2d_s2d_packed_weight_bytes(Cout, Cin, K, pad)
    taps = nbytes // (Cout * 4 * Cin * 2)
    out = torch.empty(taps, Cout, 4 * Cin, dtype=torch.bfloat16, device=w_oihw.device)
    N.check(N.lib().lss_conv2d_pack_weights_s2d(N.ptr(w_oihw), Cout, Cin, K, pad, N.ptr(out), N.stream()),
            "lss_conv2d_pack_weights_s2d")
    return out


def conv2d_s2_nhwc(x, w_s2d, K, pad, scale=None, shift=None, residual=None, relu=False, stats=None,
                   tag="conv2d_fwd"):
    """Stride-2 K x K conv (3/pad 1, 7/pad 3 with s2d-packed weights; 1/pad 0 with the plain
    pack), bf16 NHWC, on the LDS-tiled kernel."""
    B, H, W, Cx = x.shape
    taps, Cout, C4 = w_s2d.shape
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or w_s2d.dtype != torch.bfloat16 \
            or C4 != (Cx if K == 1 else 4 * Cx):
        raise ValueError("conv2d_s2_nhwc operands must be contiguous bf16 with s2d-packed weights")
    Ho, Wo = (H + 2 * pad - K) // 2 + 1, (W + 2 * pad - K) // 2 + 1
    y = torch.empty(B, Ho, Wo, Cout, dtype=torch.bfloat16, device=x.device)
    _check_per_channel(Cout, scale=scale, shift=shift)
    _check_per_channel(2 * Cout, stats=stats)
    if residual is not None and (residual.dtype != torch.bfloat16 or tuple(residual.shape) != tuple(y.shape)
                                 or not residual.is_contiguous()):
        raise ValueError("residual must match the output")
    _conv_launch(1, tag, {"x": x, "w": w_s2d, "scale": scale, "shift": shift, "residual": residual, "y": y,
                          "stats": stats},
                 B=B, H=H, W=W, Cx=Cx, Cout=Cout, KH=K, KW=K, stride=2, pad=pad, relu=1 if relu else 0)
    return y


def conv2d_s2_dual_nhwc(x, w_s2d, scale, shift, split, relu=True, tag="conv2d_fwd"):
    """Two 3x3/2 (pad 1) convs over the same bf16 NHWC input in one launch: w_s2d (taps, Cout, 4*Cx) holds
    both weight sets stacked along Cout; channels [0, split) -> y (activation applied), the rest -> y2."""
    B, H, W, Cx = x.shape
    taps, Cout, C4 = w_s2d.shape
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or w_s2d.dtype != torch.bfloat16 or C4 != 4 * Cx:
        raise ValueError("conv2d_s2_dual_nhwc operands must be contiguous bf16 with s2d-packed weights")
    _f32c(scale, "scale", (Cout,))
    _f32c(shift, "shift", (Cout,))
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty(B, Ho, Wo, split, dtype=torch.bfloat16, device=x.device)
    y2 = torch.empty(B, Ho, Wo, Cout - split, dtype=torch.bfloat16, device=x.device)
    _conv_launch(3, tag, {"x": x, "w": w_s2d, "scale": scale, "shift": shift, "y": y, "y2": y2},
                 B=B, H=H, W=W, Cx=Cx, Cout=Cout, KH=3, KW=3, stride=2, pad=1, relu=1 if relu else 0, split=split)
    return y, y2


def conv_ks_s2_dual_ok(B, H, W, Cin, Cout):
    """Is this BasicBlock entry (3x3 / stride 2 / pad 1 conv + 1x1 / stride 2 downsample, bf16, Cout channels each) a
    case for the stride-2 mode of the K-split one-pass kernel (lss_conv2d_ks_s2_dual_ok)?"""
    return bool(N.lib().lss_conv2d_ks_s2_dual_ok(B, H, W, Cin, Cout))


def pack_conv_weight_ks_s2_dual(w1_oihw, wd_oihw):
    """conv1 (Cout, Cin, 3, 3) + downsample (Cout, Cin, 1, 1) fp32 -> KsWeight in the stride-2 K-split layout."""
    Cout, Cin, KH, KW = w1_oihw.shape
    _f32c(w1_oihw, "conv weight")
    _f32c(wd_oihw, "downsample weight", (Cout, Cin, 1, 1))
    nbytes = N.lib().lss_conv2d_ks_s2_dual_packed_weight_bytes(Cout, Cin)
    if (KH, KW) != (3, 3) or nbytes == 0:
        raise ValueError("KS stride-2 weights: 3x3 + 1x1, Cout %% 64 == 0, Cin in (64, 128) (got %s)"
                         % (tuple(w1_oihw.shape),))
    out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w1_oihw.device)
    N.check(N.lib().lss_conv2d_pack_weights_ks_s2_dual(N.ptr(w1_oihw), N.ptr(wd_oihw), Cout, Cin, N.ptr(out),
                                                       N.stream()), "lss_conv2d_pack_weights_ks_s2_dual")
    return KsWeight(out, Cout, Cin)


def conv2d_ks_s2_dual_nhwc(x, w_ks, scale=None, shift=None, relu=True, tag="conv2d_fwd"):
    """relu(scale[:C] * conv3x3/2(x, w1) + shift[:C]) and scale[C:] * conv1x1/2(x, wd) + shift[C:] over the same bf16
    NHWC input in one launch of the K-split one-pass kernel; w_ks from pack_conv_weight_ks_s2_dual, scale / shift
    (2 Cout) fp32 or None.  Returns (y, y2), both (B, Ho, Wo, Cout)."""
    B, H, W, Cx = x.shape
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or not isinstance(w_ks, KsWeight) or w_ks.Cin != Cx \
            or w_ks.data.numel() != w_ks.Cout * Cx * 10:
        raise ValueError("conv2d_ks_s2_dual_nhwc operands must be contiguous bf16 with stride-2 KS-packed weights")
    Cout = w_ks.Cout
    _check_per_channel(2 * Cout, scale=scale, shift=shift)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(B, Ho, Wo, Cout, dtype=torch.bfloat16, device=x.device)
    y2 = torch.empty(B, Ho, Wo, Cout, dtype=torch.bfloat16, device=x.device)
    _conv_launch(4, tag, {"x": x, "w": w_ks.data, "scale": scale, "shift": shift, "y": y, "y2": y2},
                 B=B, H=H, W=W, Cx=Cx, Cout=Cout, KH=3, KW=3, stride=2, pad=1, relu=1 if relu else 0)
    return y, y2


def conv_ks_stem_ok(B, H, W, Cin, Cout):
    """Is this 7x7 / stride 2 / pad 3 conv (bf16, Cin 64) a case for the stem mode of the K-split one-pass kernel
    (lss_conv2d_ks_stem_ok)?"""
    return bool(N.lib().lss_conv2d_ks_stem_ok(B, H, W, Cin, Cout))


def pack_conv_weight_ks_stem(w_oihw):
    """(Cout, 64, 7, 7) fp32 -> KsWeight in the stem layout of the K-split kernel."""
    Cout, Cin, KH, KW = w_oihw.shape
    _f32c(w_oihw, "conv weight")
    nbytes = N.lib().lss_conv2d_ks_stem_packed_weight_bytes(Cout, Cin)
    if (KH, KW) != (7, 7) or nbytes == 0:
        raise ValueError("KS stem weights: 7x7, Cout %% 64 == 0, Cin 64 (got %s)" % (tuple(w_oihw.shape),))
    out = torch.empty(nbytes // 2, dtype=torch.bfloat16, device=w_oihw.device)
    N.check(N.lib().lss_conv2d_pack_weights_ks_stem(N.ptr(w_oihw), Cout, Cin, N.ptr(out), N.stream()),
            "lss_conv2d_pack_weights_ks_stem")
    return KsWeight(out, Cout, Cin)


def conv2d_ks_stem_nhwc(x, w_ks, scale=None, shift=None, relu=True, tag="conv2d_fwd"):
    """act(scale * conv7x7/2/pad3(x, w) + shift) on the stem mode of the K-split one-pass kernel: x (B, H, W, 64) bf16
    NHWC, w_ks from pack_conv_weight_ks_stem, scale / shift (Cout) fp32 or None.  Returns (B, Ho, Wo, Cout) bf16."""
    B, H, W, Cx = x.shape
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or not isinstance(w_ks, KsWeight) or w_ks.Cin != Cx \
            or w_ks.data.numel() != w_ks.Cout * Cx * 49:
        raise ValueError("conv2d_ks_stem_nhwc operands must be contiguous bf16 with stem KS-packed weights")
    Cout = w_ks.Cout
    _check_per_channel(Cout, scale=scale, shift=shift)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty(B, Ho, Wo, Cout, dtype=torch.bfloat16, device=x.device)
    _conv_launch(5, tag, {"x": x, "w": w_ks.data, "scale": scale, "shift": shift, "y": y},
                 B=B, H=H, W=W, Cx=Cx, Cout=Cout, KH=7, KW=7, stride=2, pad=3, relu=1 if relu else 0)
    return y


def conv3x3_head_nchw(x, w_packed, scale, shift, head_w, head_b, x2=None, up=1, relu=True, tag="conv2d_fwd"):
    """3x3/s1/p1 conv (+fused upsample/concat) + scale/shift + ReLU + 1x1 head in one launch.
    x (B,H,W,Cx) bf16 NHWC; head_w (n,Cout) fp32, Cout = 128 (64: plain 3x3 only); returns (B, n, H*up, W*up)
    fp32 NCHW."""
    B, H, W, Cx = x.shape
    ring = isinstance(w_packed, RingWeight)
    if ring:
        taps, Cout, Cin, w_packed = 9, w_packed.Cout, w_packed.Cin, w_packed.data
    else:
        taps, Cout, Cin = w_packed.shape
    C2 = x2.shape[3] if x2 is not None else 0
    if x.dtype != torch.bfloat16 or not x.is_contiguous() or taps != 9 or Cin != Cx + C2 or Cout not in (64, 128) \
            or (Cout == 64 and (up != 1 or C2 != 0)):
        raise ValueError("conv3x3_head_nchw: bf16 NHWC input, 3x3 weights with Cout == 128 (or 64 without "
                         "upsample / concat) required")
    n = head_w.shape[0]
    _f32c(head_w, "head_w", (n, Cout))
    _f32c(head_b, "head_b", (n,))
    _f32c(scale, "scale", (Cout,))
    _f32c(shift, "shift", (Cout,))
    out = torch.empty(B, n, H * up, W * up, dtype=torch.float32, device=x.device)
    _conv_launch(2, tag, {"x": x, "x2": x2, "w": w_packed, "scale": scale, "shift": shift, "head_w": head_w,
                          "head_b": head_b, "head_out": out},
                 B=B, H=H, W=W, Cx=Cx, C2=C2, up=up, Cout=Cout, KH=3, KW=3, stride=1, pad=1,
                 relu=(1 if relu else 0) | (W_RING if ring else 0), head_n=n)
    return out


def nchw_to_nhwc(x, dt):
    """(B,C,H,W) fp32 contiguous -> (B,H,W,C) in dt."""
    _f32c(x, "x")
    B, C, H, W = x.shape
    y = torch.empty(B, H, W, C, dtype=_TORCH_DT[dt], device=x.device)
    N.check(N.lib().lss_nchw_f32_to_nhwc(N.ptr(x), N.ptr(y), B, C, H, W, dt, N.stream()), "lss_nchw_f32_to_nhwc")
    return y


def nhwc_to_nchw(x, dt):
    """(B,H,W,C) in dt -> (B,C,H,W) fp32 contiguous."""
    if x.dtype != _TORCH_DT[dt] or not x.is_contiguous():
        raise ValueError("x must be contiguous %s" % _TORCH_DT[dt])
    B, H, W, C = x.shape
    y = torch.empty(B, C, H, W, dtype=torch.float32, device=x.device)
    N.check(N.lib().lss_nhwc_to_nchw_f32(N.ptr(x), N.ptr(y), B, C, H, W, dt, N.stream()), "lss_nhwc_to_nchw_f32")
    return y


# --- K13: the camera branch of the vovnet model at inference (csrc/camera_branch.hip) --------------------------------
def tapconv_ok(BN, H, W, Cin, Cout):
    """Does the tap-list conv kernel take (BN, H, W, Cin) -> Cout?  (lss_tapconv_ok)"""
    return N.lib().lss_tapconv_ok(int(BN), int(H), int(W), int(Cin), int(Cout)) == 1


def live_taps(H, W, ksize, dilation):
    """The taps ky * 3 + kx of a 3x3 conv with `dilation` (padding = dilation) that can reach an (H, W) map: tap
    (ky, kx) reads zero padding only when |ky d| >= H or |kx d| >= W.  A 1x1 conv has the single tap 0."""
    if ksize == 1:
        return [0]
    return [t for t in range(9) if abs((t // 3 - 1) * dilation) < H and abs((t % 3 - 1) * dilation) < W]


def tapconv(x, branches, y=None, img_bias=None, means=False, relu=True, tag="tapconv"):
    """Up to four conv branches over one NHWC bf16 input in ONE launch (lss_tapconv_fwd).

    x         (BN, H, W, Cin) bf16 contiguous
    branches  sequence of (w_packed, ksize, dilation, scale, shift, ch_off): w_packed the [tap][Cout][Cin] bf16 image of
              `pack_conv_weight` (9 taps for ksize 3, 1 for ksize 1), scale / shift (Cout) fp32 or None
    y         (BN, H, W, Cy) bf16 contiguous or None: branch b writes channels ch_off .. ch_off + Cout - 1 of it
    img_bias  (BN, Cout) fp32 or None, added in front of the folded BN (one branch only)
    means     True: also return the (BN, Cout) fp32 per-image channel means of the stored values (one branch only); with
              y = None the map itself is never written
    Returns `means` (or None)."""
    if x.dim() != 4 or x.dtype != torch.bfloat16 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError("x must be a contiguous (BN, H, W, Cin) bf16 GPU tensor")
    BN, H, W, Cin = x.shape
    branches = list(branches)
    if not 1 <= len(branches) <= 4:
        raise ValueError("1 to 4 branches per launch, got %d" % len(branches))
    Cout = branches[0][0].shape[1] if branches[0][0].dim() == 3 else -1
    if y is None and not means:
        raise ValueError("nothing to write: give y or ask for the means")
    if (img_bias is not None or means) and len(branches) != 1:
        raise ValueError("img_bias and means belong to a single branch")
    d = N.TapconvDesc()
    for b, (w, ksize, dilation, scale, shift, ch_off) in enumerate(branches):
        if ksize not in (1, 3):
            raise ValueError("branch %d: ksize must be 1 or 3" % b)
        if (w.dtype != torch.bfloat16 or not w.is_contiguous() or not w.is_cuda
                or tuple(w.shape) != (ksize * ksize, Cout, Cin)):
            raise ValueError("branch %d: weights must be a contiguous bf16 GPU [%d][%d][%d] image, got %s %s"
                             % (b, ksize * ksize, Cout, Cin, w.dtype, tuple(w.shape)))
        if int(dilation) < 1:
            raise ValueError("branch %d: dilation must be >= 1" % b)
        for name, t in (("scale", scale), ("shift", shift)):
            if t is not None:
                _f32c(t, "branch %d %s" % (b, name), (Cout,))
        if y is not None and not (0 <= ch_off and ch_off % 4 == 0 and ch_off + Cout <= y.shape[-1]):
            raise ValueError("branch %d: channels %d..%d do not fit the output" % (b, ch_off, ch_off + Cout - 1))
        br = d.branch[b]
        br.w, br.scale, br.shift = w.data_ptr(), N.ptr(scale), N.ptr(shift)
        br.ksize, br.dilation, br.ch_off = ksize, int(dilation), int(ch_off)
    if not tapconv_ok(BN, H, W, Cin, Cout):
        raise ValueError("lss_tapconv_ok refuses BN=%d H=%d W=%d Cin=%d Cout=%d" % (BN, H, W, Cin, Cout))
    if y is not None:
        if (y.dim() != 4 or y.dtype != torch.bfloat16 or not y.is_contiguous() or not y.is_cuda
                or tuple(y.shape[:3]) != (BN, H, W) or y.shape[3] % 4 != 0):
            raise ValueError("y must be a contiguous (BN, H, W, Cy) bf16 GPU tensor with Cy % 4 == 0")
    if img_bias is not None:
        _f32c(img_bias, "img_bias", (BN, Cout))
    out = torch.empty(BN, Cout, dtype=torch.float32, device=x.device) if means else None
    d.x, d.y, d.img_bias, d.means = x.data_ptr(), N.ptr(y), N.ptr(img_bias), N.ptr(out)
    d.BN, d.H, d.W, d.Cin, d.Cout, d.nbranch = BN, H, W, Cin, Cout, len(branches)
    d.y_stride, d.relu = (y.shape[3] if y is not None else 0), 1 if relu else 0
    with _timed(tag):
        N.check(N.lib().lss_tapconv_fwd(ctypes.byref(d), N.stream()), "lss_tapconv_fwd")
    return out


# --- K16: the backward halves of the tap-list conv (csrc/tapconv_wgrad.hip) ------------------------------------------
def tapconv_wgrad_ok(BN, H, W, Cin, Cout):
    """Does the tap-list weight-gradient kernel take (BN, H, W, Cin) x (BN, H, W, Cout)?  (lss_tapconv_wgrad_ok:
    lss_tapconv_ok's channel rules and H W <= 224)"""
    return N.lib().lss_tapconv_wgrad_ok(int(BN), int(H), int(W), int(Cin), int(Cout)) == 1


def _nhwc_bf16_gpu(t, name):
    if t.dim() != 4 or t.dtype != torch.bfloat16 or not t.is_contiguous() or not t.is_cuda:
        raise ValueError("%s must be a contiguous (BN, H, W, C) bf16 GPU tensor" % name)


def tapconv_wgrad(x, dy, ksize, dilation):
    """Weight gradient of a conv with ksize 1 | 3, stride 1, padding = dilation (lss_tapconv_wgrad): x (BN, H, W, Cin),
    dy (BN, H, W, Cout) contiguous bf16 NHWC -> dw (Cout, Cin, ksize, ksize) fp32, dead taps exactly 0,
    bit-reproducible.  The workspace is cached per shape and device."""
    _nhwc_bf16_gpu(x, "x")
    _nhwc_bf16_gpu(dy, "dy")
    BN, H, W, Cin = x.shape
    Cout = dy.shape[3]
    if tuple(dy.shape[:3]) != (BN, H, W):
        raise ValueError("dy %s does not match x %s" % (tuple(dy.shape), tuple(x.shape)))
    if ksize not in (1, 3) or int(dilation) < 1:
        raise ValueError("ksize must be 1 or 3 and dilation >= 1")
    if not tapconv_wgrad_ok(BN, H, W, Cin, Cout):
        raise ValueError("lss_tapconv_wgrad_ok refuses BN=%d H=%d W=%d Cin=%d Cout=%d" % (BN, H, W, Cin, Cout))
    nbytes = N.lib().lss_tapconv_wgrad_workspace_bytes(BN, H, W, Cin, Cout, ksize, int(dilation))
    ws = _cached_ws(_wgrad_ws, ("tapconv", BN, H, W, Cin, Cout, ksize, int(dilation), str(x.device)), nbytes, x.device)
    dw = torch.empty(Cout, Cin, ksize, ksize, dtype=torch.float32, device=x.device)
    with _timed("tapconv_wgrad"):
        N.check(N.lib().lss_tapconv_wgrad(N.ptr(x), N.ptr(dy), BN, H, W, Cin, Cout, ksize, int(dilation), N.ptr(ws),
                                          nbytes, N.ptr(dw), N.stream()), "lss_tapconv_wgrad")
    return dw


def tapconv_bias_grad(dz):
    """The gradient of `tapconv`'s img_bias (lss_tapconv_bias_grad): dz (BN, H, W, Cout) contiguous bf16 NHWC ->
    (BN, Cout) fp32 sums over each image's pixels, one fixed order."""
    _nhwc_bf16_gpu(dz, "dz")
    BN, H, W, Cout = dz.shape
    out = torch.empty(BN, Cout, dtype=torch.float32, device=dz.device)
    with _timed("tapconv_bias_grad"):
        N.check(N.lib().lss_tapconv_bias_grad(N.ptr(dz), BN, H, W, Cout, N.ptr(out), N.stream()),
                "lss_tapconv_bias_grad")
    return out


def camera_pool_bias(mean, wg, scale, shift, wj, want_g=False):
    """The ASPP pooling branch as a per-image bias of the projection (lss_camera_pool_bias_fwd):
    g = relu(scale * (wg . mean) + shift) (BN, Cg), bias = wj . g (BN, Cout), all fp32.  Returns bias, or (g, bias)."""
    if mean.dim() != 2 or wg.dim() != 2 or wj.dim() != 2:
        raise ValueError("mean (BN, C), wg (Cg, C) and wj (Cout, Cg) must be matrices")
    BN, C = mean.shape
    Cg, Cout = wg.shape[0], wj.shape[0]
    _f32c(mean, "mean")
    _f32c(wg, "wg", (Cg, C))
    _f32c(wj, "wj", (Cout, Cg))
    for name, t in (("scale", scale), ("shift", shift)):
        if t is not None:
            _f32c(t, name, (Cg,))
    if not (1 <= BN <= 65535 and 1 <= C <= 1024 and 1 <= Cg <= 1024 and 1 <= Cout <= 4096):
        raise ValueError("camera_pool_bias: BN=%d C=%d Cg=%d Cout=%d outside the kernel's limits" % (BN, C, Cg, Cout))
    g = torch.empty(BN, Cg, dtype=torch.float32, device=mean.device) if want_g else None
    bias = torch.empty(BN, Cout, dtype=torch.float32, device=mean.device)
    with _timed("camera_pool_bias"):
        N.check(N.lib().lss_camera_pool_bias_fwd(N.ptr(mean), N.ptr(wg), N.ptr(scale), N.ptr(shift), N.ptr(wj), BN, C, Cg,
                                                 Cout, N.ptr(g), N.ptr(bias), N.stream()), "lss_camera_pool_bias_fwd")
    return (g, bias) if want_g else bias


# --- K14: the six-token tail of the vovnet model at inference (csrc/camera_tail.hip) ---------------------------------
def camera_tail_ok(B, n_tok, n_action, n_desc):
    """Does the tail kernel take B samples of n_tok tokens and these class counts?  (lss_camera_tail_ok)"""
    return N.lib().lss_camera_tail_ok(int(B), int(n_tok), int(n_action), int(n_desc)) == 1


def bev_pool_parts(B, R):
    """The default number of row ranges `bev_pool` splits R rows into (lss_bev_pool_parts): a function of R alone."""
    parts = N.lib().lss_bev_pool_parts(int(B), int(R))
    if parts < 1:
        raise ValueError("bev_pool: B=%d R=%d outside the kernel's limits" % (B, R))
    return parts


def bev_pool(map_nhwc, parts=None):
    """Column sums of a channels-last map (lss_bev_pool_fwd): (B, ..., 256) bf16 or fp32 contiguous -> (B, P, 256) fp32,
    part p the sums over the p-th contiguous range of the R = prod(...) rows.  `partials.sum(1) / R` is the mean over
    the map; `camera_tail(..., bev=partials, bev_scale=1 / R)` takes it without another launch."""
    if (not torch.is_tensor(map_nhwc) or not map_nhwc.is_cuda or map_nhwc.dtype not in _DT or map_nhwc.dim() < 3
            or not map_nhwc.is_contiguous()):
        raise ValueError("map must be a contiguous (B, ..., 256) bf16 or fp32 GPU tensor")
    B, C = map_nhwc.shape[0], map_nhwc.shape[-1]
    R = map_nhwc[0].numel() // C if C else 0
    if C != 256 or B < 1 or R < 1:
        raise ValueError("bev_pool takes (B >= 1, R >= 1, 256) maps, got %s" % (tuple(map_nhwc.shape),))
    P = bev_pool_parts(B, R) if parts is None else int(parts)
    if not 1 <= P <= 256:
        raise ValueError("parts must be in 1..256, got %d" % P)
    partials = torch.empty(B, P, 256, dtype=torch.float32, device=map_nhwc.device)
    with _timed("bev_pool"):
        N.check(N.lib().lss_bev_pool_fwd(N.ptr(map_nhwc), _DT[map_nhwc.dtype], B, R, C, P, N.ptr(partials), N.stream()),
                "lss_bev_pool_fwd")
    return partials


def _camera_tail_shapes(n_embed, n_tok, n_action, n_desc):
    d, ff = 256, 512
    return {"cam_embed": (n_embed, d), "sa_in_w": (3 * d, d), "sa_in_b": (3 * d,), "sa_out_w": (d, d), "sa_out_b": (d,),
            "norm1_w": (d,), "norm1_b": (d,), "ffn1_w": (ff, d), "ffn1_b": (ff,), "ffn2_w": (d, ff), "ffn2_b": (d,),
            "norm2_w": (d,), "norm2_b": (d,),
            "ca_in_w": (3 * d, d), "ca_in_b": (3 * d,), "ca_out_w": (d, d), "ca_out_b": (d,), "norm3_w": (d,),
            "norm3_b": (d,),
            "cam_w": (n_tok,), "enc1_w": (ff, d), "enc1_b": (ff,), "ln1_w": (ff,), "ln1_b": (ff,), "enc2_w": (d, ff),
            "enc2_b": (d,), "ln2_w": (d,), "ln2_b": (d,), "act_w": (n_action, d), "act_b": (n_action,),
            "desc_w": (n_desc, d), "desc_b": (n_desc,)}


def camera_tail(tokens, params, bev=None, bev_scale=1.0):
    """camera_transformer -> bev_fusion -> unified_predictor at inference in ONE launch (lss_camera_tail_fwd).

    tokens  (B, N <= 8, 256) fp32 contiguous
    params  {field of lss_camera_tail_desc_t: fp32 contiguous GPU tensor}, read in place, plus the floats "eps_cam",
            "eps_fuse", "eps_pred" (default 1e-5) and optionally "ids" (B, N) int64 (default 0 .. N-1).  The 13 operands of
            the camera transformer (`N.CameraTailDesc.CAMERA`) and the 6 of the fusion (`.FUSION`) are each given whole
            or left out (the stage is then skipped); the predictor's 13 are required.
    bev     with the fusion: the pooled BEV token (B, 256), or `bev_pool`'s partials (B, P, 256) with bev_scale = 1 / R
    Returns (action (B, n_action), description (B, n_desc)), fp32."""
    if not torch.is_tensor(tokens) or tokens.dim() != 3 or tokens.shape[2] != 256:
        raise ValueError("tokens must be (B, N, 256)")
    _f32c(tokens, "tokens")
    B, n_tok = tokens.shape[0], tokens.shape[1]
    D = N.CameraTailDesc
    missing = [k for k in D.PREDICTOR if params.get(k) is None]
    if missing:
        raise ValueError("camera_tail: the predictor's operands are required, missing %s" % missing)
    if params["act_w"].dim() != 2 or params["desc_w"].dim() != 2:
        raise ValueError("act_w and desc_w must be matrices")
    n_action, n_desc = params["act_w"].shape[0], params["desc_w"].shape[0]
    if B < 1 or not camera_tail_ok(B, n_tok, n_action, n_desc):
        raise ValueError("lss_camera_tail_ok refuses B=%d N=%d n_action=%d n_desc=%d" % (B, n_tok, n_action, n_desc))
    stages = []
    for group in (D.CAMERA, D.FUSION):
        given = [k for k in group if params.get(k) is not None]
        if given and len(given) != len(group):
            raise ValueError("camera_tail: a stage is given whole or not at all, got only %s" % given)
        stages.append(bool(given))
    with_cam, with_fusion = stages
    n_embed = params["cam_embed"].shape[0] if with_cam and params["cam_embed"].dim() == 2 else 0
    shapes = _camera_tail_shapes(n_embed, n_tok, n_action, n_desc)
    d = D()
    names = D.PREDICTOR + (D.CAMERA if with_cam else ()) + (D.FUSION if with_fusion else ())
    for k in names:
        t = _f32c(params[k], k, shapes[k])
        if t.device != tokens.device:
            raise ValueError("%s lives on %s, the tokens on %s" % (k, t.device, tokens.device))
        setattr(d, k, t.data_ptr())
    ids = params.get("ids") if with_cam else None
    if ids is not None:
        if (ids.dtype != torch.int64 or not ids.is_cuda or not ids.is_contiguous()
                or tuple(ids.shape) != (B, n_tok)):
            raise ValueError("ids must be a contiguous (B, N) int64 GPU tensor")
        d.ids = ids.data_ptr()
    elif with_cam and n_embed < n_tok:
        raise ValueError("cam_embed has %d rows for %d tokens" % (n_embed, n_tok))
    if with_fusion:
        if bev is None or bev.dim() not in (2, 3):
            raise ValueError("the fusion needs bev (B, 256) or (B, P, 256)")
        P = 1 if bev.dim() == 2 else bev.shape[1]
        _f32c(bev, "bev", (B, 256) if bev.dim() == 2 else (B, P, 256))
        if not 1 <= P <= 256 or bev.device != tokens.device:
            raise ValueError("bev: 1..256 parts on the tokens' device")
        d.bev, d.bev_parts, d.bev_scale = bev.data_ptr(), P, float(bev_scale)
    action = torch.empty(B, n_action, dtype=torch.float32, device=tokens.device)
    description = torch.empty(B, n_desc, dtype=torch.float32, device=tokens.device)
    d.tokens, d.action, d.description = tokens.data_ptr(), action.data_ptr(), description.data_ptr()
    d.eps_cam, d.eps_fuse, d.eps_pred = (float(params.get(k, 1e-5)) for k in ("eps_cam", "eps_fuse", "eps_pred"))
    d.B, d.N, d.n_embed, d.n_action, d.n_desc = B, n_tok, n_embed, n_action, n_desc
    with _timed("camera_tail"):
        N.check(N.lib().lss_camera_tail_fwd(ctypes.byref(d), N.stream()), "lss_camera_tail_fwd")
    return action, description


# --- K15: the TXT half of BEV_TXT at inference behind the ASPP (csrc/txt_heads.hip) ----------------------------------
def bev_post(bev, origin, size, weight, scale, shift):
    """BevPost on a crop of `bev`, read in place (lss_bev_post_fwd): 3x3 conv, stride (2, 1), padding 1 around the CROP
    -> scale / shift -> ReLU -> MaxPool (5, 4).

    bev     (B, Cb <= 8, Hm, Wm) fp32 GPU tensor in ANY layout (its strides go to the kernel; nothing is copied)
    origin  (h0, w0) and size (Hc, Wc) of the crop
    weight  (Co <= 16, Cb, 3, 3) fp32 contiguous; scale / shift (Co) fp32
    Returns (B, Co, (((Hc - 1) // 2) + 1) // 5, Wc // 4) fp32."""
    if not torch.is_tensor(bev) or bev.dim() != 4 or bev.dtype != torch.float32 or not bev.is_cuda:
        raise ValueError("bev must be a (B, Cb, Hm, Wm) fp32 GPU tensor")
    B, Cb, Hm, Wm = bev.shape
    (h0, w0), (Hc, Wc) = (int(v) for v in origin), (int(v) for v in size)
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (Cb, 3, 3):
        raise ValueError("weight must be (Co, %d, 3, 3), got %s" % (Cb, tuple(weight.shape)))
    Co = weight.shape[0]
    _f32c(weight, "weight")
    _f32c(scale, "scale", (Co,))
    _f32c(shift, "shift", (Co,))
    if not (0 <= h0 and 0 <= w0 and 1 <= Hc and 1 <= Wc and h0 + Hc <= Hm and w0 + Wc <= Wm):
        raise ValueError("the crop (%d, %d) + (%d, %d) leaves the %d x %d map" % (h0, w0, Hc, Wc, Hm, Wm))
    Ho, Wo = (((Hc - 1) // 2) + 1) // 5, Wc // 4
    if not (1 <= B <= 65535 and 1 <= Cb <= 8 and 1 <= Co <= 16 and Ho >= 1 and Wo >= 1):
        raise ValueError("bev_post: B=%d Cb=%d Co=%d crop %dx%d outside the kernel's limits" % (B, Cb, Co, Hc, Wc))
    y = torch.empty(B, Co, Ho, Wo, dtype=torch.float32, device=bev.device)
    sb, sc, sh, sw = bev.stride()
    with _timed("bev_post"):
        N.check(N.lib().lss_bev_post_fwd(N.ptr(bev), sb, sc, sh, sw, Hm, Wm, h0, w0, B, Cb, Hc, Wc, N.ptr(weight),
                                         N.ptr(scale), N.ptr(shift), Co, N.ptr(y), N.stream()), "lss_bev_post_fwd")
    return y


def txt_heads_ok(B, ncams, n_slots, H, W, Cp, E, n_act, n_desc_f):
    """Does K15 take these sizes?  (lss_txt_heads_ok)"""
    return N.lib().lss_txt_heads_ok(int(B), int(ncams), int(n_slots), int(H), int(W), int(Cp), int(E), int(n_act),
                                    int(n_desc_f)) == 1


TXT_HEADS_CAMS = (1, 0, 3, 2, 5)  # front, then the reference's side order l1, l2, r1, r2 (model_BEV_TXT.py:293-332)
_txt_heads_ws = {}


def txt_heads(scene, bev_post_map, front, side, predictors, cams=TXT_HEADS_CAMS, ncams=6):
    """Everything behind the scene map in two launches (lss_txt_heads_fwd).

    scene         (B * ncams, H, W, 256) bf16 contiguous
    bev_post_map  (B, Cp <= 8, H, W) fp32 contiguous
    front, side   (embed_w [9][32][256] bf16 image, embed_scale (32), embed_shift (32), lin_w (E, (32 + Cp) H W),
                  lin_b (E)): slot 0 takes `front`, every other slot `side` (None when there is one slot)
    predictors    {"f1_w": (n_desc_f, E), "f1_b", "f2_w": (n_act, E), "f2_b", "lr_w": (1, E), "lr_b"} fp32, read in place
    cams          the camera of each slot
    Returns (act (B, n_act), desc (B, n_desc_f + len(cams) - 1)) fp32."""
    if (not torch.is_tensor(scene) or scene.dim() != 4 or scene.dtype != torch.bfloat16 or not scene.is_contiguous()
            or not scene.is_cuda or scene.shape[3] != 256):
        raise ValueError("scene must be a contiguous (B * ncams, H, W, 256) bf16 GPU tensor")
    BN, H, W, _ = scene.shape
    cams = tuple(int(c) for c in cams)
    ncams, n_slots = int(ncams), len(cams)
    if ncams < 1 or BN % ncams != 0 or not 1 <= n_slots <= 8 or any(not 0 <= c < ncams for c in cams):
        raise ValueError("txt_heads: %d images, ncams=%d, slots %s" % (BN, ncams, cams))
    B = BN // ncams
    if bev_post_map.dim() != 4 or tuple(bev_post_map.shape[0:1] + bev_post_map.shape[2:]) != (B, H, W):
        raise ValueError("bev_post must be (%d, Cp, %d, %d), got %s" % (B, H, W, tuple(bev_post_map.shape)))
    _f32c(bev_post_map, "bev_post")
    Cp = bev_post_map.shape[1]
    if front[3].dim() != 2 or predictors["f1_w"].dim() != 2 or predictors["f2_w"].dim() != 2:
        raise ValueError("lin_w, f1_w and f2_w must be matrices")
    E, n_desc_f, n_act = front[3].shape[0], predictors["f1_w"].shape[0], predictors["f2_w"].shape[0]
    if not txt_heads_ok(B, ncams, n_slots, H, W, Cp, E, n_act, n_desc_f):
        raise ValueError("lss_txt_heads_ok refuses B=%d ncams=%d slots=%d H=%d W=%d Cp=%d E=%d n_act=%d n_desc_f=%d"
                         % (B, ncams, n_slots, H, W, Cp, E, n_act, n_desc_f))
    if n_slots > 1 and side is None:
        raise ValueError("side slots need the side set")
    d = N.TxtHeadsDesc()
    for name, group, dst in (("front", front, d.front), ("side", side if n_slots > 1 else None, d.side)):
        if group is None:
            continue
        ew, esc, esh, lw, lb = group
        if (ew.dtype != torch.bfloat16 or not ew.is_contiguous() or not ew.is_cuda or tuple(ew.shape) != (9, 32, 256)):
            raise ValueError("%s: embed_w must be a contiguous bf16 GPU [9][32][256] image, got %s %s"
                             % (name, ew.dtype, tuple(ew.shape)))
        _f32c(esc, name + " embed_scale", (32,))
        _f32c(esh, name + " embed_shift", (32,))
        _f32c(lw, name + " lin_w", (E, (32 + Cp) * H * W))
        _f32c(lb, name + " lin_b", (E,))
        dst.embed_w, dst.embed_scale, dst.embed_shift = ew.data_ptr(), esc.data_ptr(), esh.data_ptr()
        dst.lin_w, dst.lin_b = lw.data_ptr(), lb.data_ptr()
    shapes = {"f1_w": (n_desc_f, E), "f1_b": (n_desc_f,), "f2_w": (n_act, E), "f2_b": (n_act,), "lr_w": (1, E),
              "lr_b": (1,)}
    for k in N.TxtHeadsDesc.PREDICTORS:
        if k.startswith("lr") and n_slots == 1:
            continue
        t = _f32c(predictors[k], k, shapes[k])
        if t.device != scene.device:
            raise ValueError("%s lives on %s, the scene map on %s" % (k, t.device, scene.device))
        setattr(d, k, t.data_ptr())
    nbytes = N.lib().lss_txt_heads_workspace_bytes(B, n_slots, H, W, E)
    ws = _cached_ws(_txt_heads_ws, (str(scene.device), nbytes), nbytes, scene.device)
    act = torch.empty(B, n_act, dtype=torch.float32, device=scene.device)
    desc = torch.empty(B, n_desc_f + n_slots - 1, dtype=torch.float32, device=scene.device)
    d.scene, d.bev_post, d.workspace, d.workspace_bytes = scene.data_ptr(), bev_post_map.data_ptr(), ws.data_ptr(), nbytes
    d.act, d.desc = act.data_ptr(), desc.data_ptr()
    for s, c in enumerate(cams):
        d.cams[s] = c
    d.B, d.ncams, d.n_slots, d.H, d.W, d.Cp, d.E, d.n_act, d.n_desc_f = B, ncams, n_slots, H, W, Cp, E, n_act, n_desc_f
    with _timed("txt_heads"):
        N.check(N.lib().lss_txt_heads_fwd(ctypes.byref(d), N.stream()), "lss_txt_heads_fwd")
    return act, desc
