"""fp64 references, DERIVED error bounds, cases, the launch plan and planted errors for the per-element tests of the
backward half of BevEncode's convs - tests/test_conv_wgrad_gpu.py on the GPU, tests/test_conv_wgrad_ref_cpu.py for this
helper itself.  Everything here is fp64 (or an explicit float32 emulation) on the CPU; u = 2^-24; no bound is measured
on a kernel.  `check`, `NotExercised`, `bf16_round` and `errors` are those of depth_head_ref / train_node_ref, the
exact align_corners coordinates and the corner-range arithmetic of the blend those of conv_fwd_ref.

  K9w            csrc/conv_wgrad.hip    ops.conv3x3_wgrad, ops.conv4x4_wgrad        wgrad_reference / wgrad_by_taps
  reduce         csrc/conv_grad.hip     wgrad_reduce_kernel (behind every form)     the same (split counts from the plan)
  GEMM fallback  conv_grad.hip + linear_mfma.hip   LSS_WGRAD_DIRECT=0               the same
  stride 2       modules.conv_s2_wgrad_phase_planes + _s2_wgrad_gather              s2_wgrad_reference / s2_wgrad_by_taps
  concat         csrc/conv_grad.hip     ops.upsample_cat_nhwc                       up_reference(...).cat
  adjoint        csrc/conv_grad.hip     ops.upsample_bwd_nhwc (walk, rows<8>, rows<12>)   up_reference(...).dx

Weight gradient.  dW[co][ci][ty][tx] = sum_{b,y,x} dY[b,y,x,co] X[b, y + d_ty, x + d_tx, ci] over the in-image terms,
displacements d in {-1, 0, 1} (3x3 / pad 1) or {-2 .. 1} (the 4x4-tap form of the 7x7 / 2 stem over phase planes);
the stride-2 forms read X[b, 2 y + ky - K // 2, 2 x + kx - K // 2].  Two derivations: torch.nn.grad.conv2d_weight on
.double() operands, and the sum written out tap by tap (which also returns S = the same sum over |dY| |X| and n = the
number of in-image terms of the tap, and holds the planted errors).
  EXACT   x integer in [-3, 3], dY integer in [-2, 2] (exact in bf16): every product and every partial sum is an integer
          of magnitude <= 6 B H W < 2^24 (asserted for every case), so an fp32 evaluation in ANY order - any row range,
          any number of partial tiles, either reduce loop, the split-K GEMM - gives the fp64 value's bits.
  BOUND   bf16-rounded randn operands.  Any fp32 evaluation of an n-term sum of exact products satisfies
          |dw - ref| <= (n + 2) u S elementwise (depth_head_ref: Higham's gamma_n S; the products of two bf16 values
          are exact in fp32).  Such a bound sees a single missing term only while (n + 2) u S stays below a typical
          product, so the bound cases keep B H W <= 2000; the exact cases carry the large shapes.

The launch plan.  `wgrad_plan` repeats conv_wgrad.hip's wgrad_plan (K blocks per row, row slots, padded rows per split,
splits; LSS_WGRAD_SPLITS included); every case states the plan facts it exists for and `plan_of` asserts them, so a
case cannot drift onto another path silently.  The GPU test holds `nsplit` against the library's workspace size.

Upsample + concat and its adjoint.  out = [x2 | A_y x A_x^T], dx = A_y^T g[..., c_off : c_off + Cx] A_x with
A[Y, y] = hat(sY - y), sY = Y (H - 1) / (up H - 1) (align_corners), built from conv_fwd_ref's exact integer coordinates.
  EXACT   up = 3, H, W in {3, 11, 43}: the ratios are 1/4, 5/16, 21/64, so fl(r), fl(r Y) and the fractions are exact,
          the weights are multiples of 2^-6, their products of 2^-12, and with integer x, g in [-3, 3] every partial sum
          is a multiple of 2^-12 below 2^7: exact in fp32.  `cat_f32` / `adjoint_f32` evaluate the kernels' own fp32
          formulas (upsample_cat_kernel's two-level blend; the adjoint's candidate window, wy * wx and fmaf chain in
          its order) and `up_reference` asserts that they equal the fp64 values bit for bit.  The kernel must then
          equal the fp64 value rounded once to bf16.  x2 and the first C2 channels of g hold the sentinel 64.
  BOUND   coordinates: the kernels take sY' = fl(fl(r) Y): two fp32 roundings, |sY' - sY| <= 2 u sY (1 + u)
          <= delta = 2.1 u (H - 1) per axis (conv_fwd_ref's derivation without its 16-bit quantisation: these kernels
          keep the fp32 fraction; y0 = (int) sY' and sY' - y0 are exact).
          adjoint: hat is 1-Lipschitz, so a weight w_y moves by at most delta_y + u (the rounding of 1 - l) even where
          the integer cell differs, and the product weight fl(w_y w_x) by at most delta_y + delta_x + 4 u (weights
          <= 1).  A CANDIDATE is a high-res pixel whose true coordinates lie within 1 + delta of (y, x) on both axes -
          every pixel that has, or can be computed to have, a non-zero weight; n = their number.  The fmaf chain over
          them in any order:
              E = sum_candidates |g| (delta_y + delta_x + 4 u) + (n + 2) u sum w |g|.
          concat (two-level form  (1 - ly) ((1 - lx) a + lx b) + ly ((1 - lx) c + lx d)):  the interpolant is
          continuous and piecewise linear, inside a cell |dv / dl| <= the range of the four corners, near a cell edge
          the 4 x 4 neighbourhood's (conv_fwd_ref.blend64).  Arithmetic: 1 - lx carries u, each product u qmax, the
          inner sum u qmax: top and bot 4 u qmax each, which the outer convex combination passes on as 4 u qmax;
          1 - ly, two products and the outer sum add 4 u qmax more (FMA contraction only removes roundings):
              dv = (delta_y + delta_x + 2 u) range + 10 u qmax    (8 counted, 2 for the second-order terms).
          output: one bf16 rounding:  |got - ref| <= E + half a bf16 ulp of (|ref| + E)   (bf16_out_bound).
`adjoint_form` repeats the host's selection (span = ceil(2 / fl(rx)) + 3: rows<8>, rows<12> or the walk).

Planted errors (`plant=`): a deliberately wrong copy of the hand-written reference.  `exercised` raises `NotExercised`
when a plant moves no element of a case by more than the case's bound (for an exact case: moves nothing).
"""
import collections
import functools
import os

import numpy as np
import torch
from torch.nn import functional as F

import conv_fwd_ref as C
from depth_head_ref import NotExercised, U32, check  # noqa: F401  (re-exported)
from train_node_ref import bf16_round, errors  # noqa: F401
from transformer_gemm_ref import bf16_out_bound, bf16_rn

WGRAD_PLANTS = ("one_position_dropped", "row_wrap", "image_boundary_leak", "last_column_dropped",
                "last_k_block_dropped", "ky_kx_swapped", "channel_tiles_swapped", "last_split_dropped")
W4_PLANTS = ("taps4x4_shifted", "tap_rows_swapped")
S2_PLANTS = ("phase_swapped", "k1_wrong_phase")
UP_PLANTS = ("adjoint_not_align_corners", "adjoint_last_row_clamp", "adjoint_window_one_short", "c_off_ignored")
PLANTS = WGRAD_PLANTS + W4_PLANTS + S2_PLANTS + UP_PLANTS
DISP = {3: (-1, 0, 1), 4: (-2, -1, 0, 1)}   # tap displacements of the two stride-1 forms

# ----------------------------------------------------------------------------------------------------------------------
# the launch plan (csrc/conv_wgrad.hip: wgrad_plan)
# ----------------------------------------------------------------------------------------------------------------------
WK_NDB, WK_MAXKB, WK_MAXXS = 10, 7, 8
WK_ROOM = 160 * 1024 - 64 * 4 - WK_NDB * 32 * 128   # LDS left for the X row slots
assert WK_ROOM == 122624
Plan = collections.namedtuple("Plan", "KB nxs rows_total rows_per nsplit tiles")


def wgrad_plan(B, H, W, Cin, Cout, splits=None):
    """The direct kernel's plan, or None where lss_conv2d_wgrad takes the GEMM fallback.  splits: LSS_WGRAD_SPLITS
    (None: the environment's, else the default of one workgroup per CU)."""
    if B <= 0 or H <= 0 or W < 8 or Cin <= 0 or Cout <= 0 or Cin % 64 or Cout % 64:
        return None
    KB = (W + 31) // 32
    if KB > WK_MAXKB:
        return None
    nxs = min(WK_MAXXS, WK_ROOM // ((32 * KB + 8) * 128))
    if nxs < 4:
        return None
    rows_total = B * (H + 2)
    tiles = (Cin // 64) * (Cout // 64)
    ns = 256 // tiles
    if splits is None and "LSS_WGRAD_SPLITS" in os.environ:
        splits = int(os.environ["LSS_WGRAD_SPLITS"])
    if splits is not None:
        ns = splits
    ns = max(ns, 1)
    per = max(3, -(-rows_total // ns))
    return Plan(KB, nxs, rows_total, per, -(-rows_total // per), tiles)


assert [wgrad_plan(1, 1, 32 * kb, 64, 64).nxs for kb in range(1, 8)] == [8, 8, 8, 7, 5, 4, 4]

# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name taps B H W Cin Cout splits facts bound")


def _w(taps, B, H, W, Cin, Cout, splits=None, bound=False, **facts):
    name = "w%d_%dx%dx%d_c%d_%d_%s" % (taps, B, H, W, Cin, Cout, "d" if splits is None else "s%d" % splits)
    return Case(name, taps, B, H, W, Cin, Cout, splits, facts, bound)


# ops.conv3x3_wgrad.  facts: what the case exists for, asserted by `plan_of` (phases = the start rows of the splits
# modulo the H + 2 period; last_split_rows = the padded rows of the last split, (image, padded row); x_rows / dy_blocks
# = what the loaders of the longest split move through the two rings)
W3_CASES = [
    # one split of three rows; one K block with 24 zero-filled positions; rows ky = 0, 2 are dead: exact zeros
    _w(3, 1, 1, 8, 64, 64, KB=1, nxs=8, rows_per=3, nsplit=1),
    # four 3-row ranges starting at every phase of the period; W no multiple of 8; two Cout tiles
    _w(3, 3, 2, 9, 64, 128, bound=True, KB=1, nsplit=4, rows_per=3, phases=[0, 1, 2, 3], tiles=2),
    # one range with four image boundaries inside; the second K block has one live position; 27 rows through eight
    # slots and 30 dY blocks through the ring of 10: both wrap three times
    _w(3, 5, 3, 33, 128, 64, 1, bound=True, KB=2, nxs=8, nsplit=1, rows_per=25, x_rows=27, dy_blocks=30),
    _w(3, 4, 7, 129, 64, 64, 1, KB=5, nxs=5, nsplit=1, rows_per=36),
    _w(3, 3, 6, 161, 64, 64, 2, KB=6, nxs=4, nsplit=2),
    _w(3, 2, 5, 224, 64, 192, 1, KB=7, nxs=4, nsplit=1, tiles=3),       # the widest row; three Cout tiles
    # six channel tiles; the eighth split holds only the last image's bottom pad row: its partial tiles are zeros
    # (also a bound case, B H W = 1800: the only one with two tiles in both channel dimensions)
    _w(3, 2, 9, 100, 192, 128, bound=True, KB=4, nxs=7, tiles=6, rows_per=3, nsplit=8, last_split_rows=[(1, 10)]),
    _w(3, 1, 46, 40, 64, 64, nsplit=16),                                  # the reduce kernel's 16-way body alone
    _w(3, 2, 30, 40, 64, 64, nsplit=22),                                  # body plus tail
    _w(3, 1, 40, 97, 64, 64, KB=4, nxs=7, nsplit=14),                     # tail alone
]
# ops.conv4x4_wgrad (taps {-2 .. 1}^2, two launches)
W4_CASES = [
    _w(4, 1, 1, 8, 64, 64, KB=1, nsplit=1),                               # every tap with dy != 0 is dead
    _w(4, 3, 2, 9, 64, 64, bound=True, nsplit=4, phases=[0, 1, 2, 3]),
    _w(4, 4, 5, 129, 64, 128, 1, KB=5, nxs=5, nsplit=1),
    _w(4, 2, 3, 224, 128, 64, 1, KB=7, nxs=4, nsplit=1),
    _w(4, 2, 30, 40, 64, 64, nsplit=22),
]
# LSS_WGRAD_DIRECT=0: (B, H, W, Cin, Cout); the last three are shapes only this path takes
GEMM_CASES = [(c.B, c.H, c.W, c.Cin, c.Cout) for c in W3_CASES[:3]] + [(2, 4, 5, 64, 64), (1, 3, 230, 64, 64),
                                                                      (2, 6, 10, 72, 40)]
GEMM_ONLY = GEMM_CASES[3:]

S2Case = collections.namedtuple("S2Case", "name K B H W C Co facts bound")
# modules.conv_s2_wgrad_phase_planes: (K, B, H, W, C, Co); the plan is that of the phase planes (B, H/2, W/2, 4 C, Co)
S2_CASES = [
    S2Case("s2_k3_2x6x18", 3, 2, 6, 18, 16, 64, dict(KB=1), True),
    S2Case("s2_k1_3x4x16", 1, 3, 4, 16, 32, 128, dict(KB=1, tiles=4), True),    # (bound too: the only K = 1 case)
    S2Case("s2_k7_2x6x22", 7, 2, 6, 22, 16, 64, dict(KB=1), True),
    S2Case("s2_k7_1x2x16", 7, 1, 2, 16, 64, 128, dict(KB=1, tiles=8, nsplit=1), False),   # one phase-plane row
    S2Case("s2_k3_1x10x66", 3, 1, 10, 66, 16, 64, dict(KB=2), False),
]
WCASES = {c.name: c for c in W3_CASES + W4_CASES}
S2_BY_NAME = {c.name: c for c in S2_CASES}
assert len(WCASES) == len(W3_CASES) + len(W4_CASES)

UpCase = collections.namedtuple("UpCase", "name B H W Cx C2 up exact")
UP_CASES = [UpCase("up3_%dx%dx%d_c%d_%d" % s, *s, 3, True) for s in
            [(2, 3, 3, 8, 0), (1, 3, 11, 64, 8), (2, 11, 11, 16, 64), (1, 11, 43, 8, 0)]] + \
           [UpCase("up%d_%dx%dx%d_c%d_%d" % ((s[5],) + s[:5]), *s, False) for s in
            [(2, 2, 2, 8, 0, 2), (1, 7, 9, 64, 64, 2), (1, 100, 100, 8, 0, 2), (2, 25, 25, 16, 8, 4), (1, 2, 5, 8, 8, 4)]]
UP_BY_NAME = {c.name: c for c in UP_CASES}
SENTINEL = 64.0


def plan_of(c):
    """The plan of a stride-1 or stride-2 case, with the facts its table line states asserted."""
    if isinstance(c, S2Case):
        B, H, W, Cin, Cout, splits = c.B, c.H // 2, c.W // 2, 4 * c.C, c.Co, None
    else:
        B, H, W, Cin, Cout, splits = c.B, c.H, c.W, c.Cin, c.Cout, c.splits
    p = wgrad_plan(B, H, W, Cin, Cout, splits)
    assert p is not None, c.name
    HP = H + 2
    for k, v in c.facts.items():
        if k == "phases":
            got = sorted({(s * p.rows_per) % HP for s in range(p.nsplit)})
        elif k == "last_split_rows":
            got = [divmod(pi, HP) for pi in range((p.nsplit - 1) * p.rows_per, p.rows_total)]
        elif k == "x_rows":      # rows pi0 - 1 .. pi0 + ntile of the longest split
            got = min(p.rows_per, p.rows_total) + 2
        elif k == "dy_blocks":   # K blocks of the real rows of a split that holds every image
            assert p.nsplit == 1
            got = B * H * p.KB
        else:
            got = getattr(p, k)
        assert got == v, (c.name, k, got, v)
    return p


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)))


def _ints(shape, g, lim):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def make_pair(name, shape_x, shape_dy, exact):
    """(x, dy) fp32 NHWC tensors of bf16 values: integers in [-3, 3] / [-2, 2], or bf16-rounded randn."""
    g = _gen(name + ("" if exact else "_bound"))
    if exact:
        return _ints(shape_x, g, 3), _ints(shape_dy, g, 2)
    return bf16_round(torch.randn(shape_x, generator=g)), bf16_round(torch.randn(shape_dy, generator=g))


@functools.lru_cache(maxsize=None)
def wgrad_operands(name, exact=True):
    """Cached: shared, never written to."""
    c = WCASES[name]
    assert exact or c.bound, name
    return make_pair(name, (c.B, c.H, c.W, c.Cin), (c.B, c.H, c.W, c.Cout), exact)


@functools.lru_cache(maxsize=None)
def s2_operands(name, exact=True):
    c = S2_BY_NAME[name]
    assert exact or c.bound, name
    return make_pair(name, (c.B, c.H, c.W, c.C), (c.B, c.H // 2, c.W // 2, c.Co), exact)


# ----------------------------------------------------------------------------------------------------------------------
# the weight gradient
# ----------------------------------------------------------------------------------------------------------------------
WRef = collections.namedtuple("WRef", "dw S n bound")


def assert_exact_precondition(x, dy):
    """Integer operands within [-3, 3] / [-2, 2] and 6 B H W < 2^24: every partial sum is an fp32 integer."""
    assert bool((x == x.round()).all()) and bool((dy == dy.round()).all())
    assert float(x.abs().max()) <= 3 and float(dy.abs().max()) <= 2
    assert 6 * dy.shape[0] * dy.shape[1] * dy.shape[2] < 2 ** 24


def wgrad_reference(x, dy, taps=3):
    """dW (Cout, Cin, taps, taps) fp64 by torch.nn.grad.conv2d_weight.  x (B,H,W,Cin), dy (B,H,W,Cout).  The 4x4 form is
    the dense 4x4 evaluation with padding left / top 2, right / bottom 1."""
    xn, dyn = x.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2)
    shape = (dy.shape[3], x.shape[3], taps, taps)
    if taps == 3:
        return torch.nn.grad.conv2d_weight(xn, shape, dyn, padding=1)
    return torch.nn.grad.conv2d_weight(F.pad(xn, (2, 1, 2, 1)), shape, dyn)


def _shift_rows(x, d, leak=False):
    """x (B,H,W,C) read at row y + d: zeros outside the image; leak: outside the whole batch only."""
    B, H, W, Ch = x.shape
    if leak:
        return _shift_rows(x.reshape(1, B * H, W, Ch), d).reshape(B, H, W, Ch)
    out = torch.zeros_like(x)
    lo, hi = max(0, -d), min(H, H - d)
    if lo < hi:
        out[:, lo:hi] = x[:, lo + d:hi + d]
    return out


def _shift_cols(x, d, wrap=False):
    """x (B,H,W,C) read at column x + d: zeros outside the row; wrap: the index is formed on the flattened image."""
    B, H, W, Ch = x.shape
    if wrap:
        return _shift_cols(x.reshape(B, 1, H * W, Ch), d).reshape(B, H, W, Ch)
    return _shift_rows(x.transpose(1, 2), d).transpose(1, 2)


def wgrad_by_taps(x, dy, taps=3, plant=None, plan=None):
    """The same sum written out tap by tap -> (dw, S, n): S = the sum over |dY| |X|, n (taps, taps) = the in-image
    terms of each tap.  plant: one of WGRAD_PLANTS / W4_PLANTS (plan: the case's launch plan, for the plants that
    name a K block or a split)."""
    if plant is not None and plant not in WGRAD_PLANTS + W4_PLANTS:
        raise NotExercised("not a plant of the stride-1 weight gradient")
    if plant in W4_PLANTS and taps != 4:
        raise NotExercised("not the 4x4-tap form")
    x, dy = x.double(), dy.double()
    B, H, W, Cin = x.shape
    Cout = dy.shape[3]
    disp = DISP[taps]
    if plant == "taps4x4_shifted":
        disp = tuple(d + 1 for d in disp)
    dyp = dy
    if plant == "last_column_dropped":
        dyp = dy.clone()
        dyp[:, :, W - 1] = 0
    if plant == "last_k_block_dropped":
        dyp = dy.clone()
        dyp[:, :, 32 * (plan.KB - 1):] = 0
    if plant == "last_split_dropped":   # padded rows from the last split's first on: (image b, row y) is row b (H + 2) + y + 1
        pi = (torch.arange(B).view(B, 1) * (H + 2) + torch.arange(H).view(1, H) + 1)
        dyp = dy * (pi < (plan.nsplit - 1) * plan.rows_per).double().view(B, H, 1, 1)
    if plant == "image_boundary_leak" and B < 2:
        raise NotExercised("no image before")
    dw = torch.zeros(Cout, Cin, taps, taps, dtype=torch.float64)
    S = torch.zeros_like(dw)
    n = torch.zeros(taps, taps, dtype=torch.float64)
    for ty, d_y in enumerate(disp):
        xr = _shift_rows(x, d_y, leak=plant == "image_boundary_leak" and d_y < 0)
        for tx, d_x in enumerate(disp):
            xs = _shift_cols(xr, d_x, wrap=plant == "row_wrap" and d_x < 0)
            dw[:, :, ty, tx] = torch.einsum("byxo,byxc->oc", dyp, xs)
            S[:, :, ty, tx] = torch.einsum("byxo,byxc->oc", dy.abs(), _shift_cols(_shift_rows(x, d_y), d_x).abs())
            n[ty, tx] = B * max(0, H - abs(d_y)) * max(0, W - abs(d_x))
    if plant == "one_position_dropped":   # the centre tap loses the last image's last row, middle column
        c0 = disp.index(0)
        dw[:, :, c0, c0] -= torch.outer(dy[B - 1, H - 1, W // 2], x[B - 1, H - 1, W // 2])
    if plant == "ky_kx_swapped":
        dw = dw.transpose(2, 3).contiguous()
    if plant == "channel_tiles_swapped":
        if Cout < 128 or Cin < 128:
            raise NotExercised("one channel tile in a dimension")
        dw = dw.clone()
        a, b = dw[:64, 64:128].clone(), dw[64:128, :64].clone()
        dw[:64, 64:128], dw[64:128, :64] = b, a
    if plant == "tap_rows_swapped":
        dw = torch.cat([dw[:, :, 2:], dw[:, :, :2]], 2)
    return dw, S, n


def wgrad_bound(S, n, exact):
    return torch.zeros_like(S) if exact else (n + 2.0) * U32 * S


def exercised(planted, ref, bound, what):
    """Raises NotExercised when the plant moves no element by more than the bound."""
    if not bool(((planted - ref).abs() > bound).any()):
        raise NotExercised("%s: the effect is inside the case's bound" % what)
    return planted


def wgrad_case_reference(x, dy, taps, exact, plan=None, plant=None):
    """WRef of a pair of operands; with `plant` the planted dw (after `exercised`) with the UNPLANTED bound."""
    dw, S, n = wgrad_by_taps(x, dy, taps)
    if exact:
        assert_exact_precondition(x, dy)
        assert float(S.max()) <= 6 * x.shape[0] * x.shape[1] * x.shape[2]
    bound = wgrad_bound(S, n, exact)
    if plant is not None:
        dw = exercised(wgrad_by_taps(x, dy, taps, plant, plan)[0], dw, bound, plant)
    return WRef(dw, S, n, bound)


@functools.lru_cache(maxsize=None)
def wgrad_ref(name, exact=True):
    """The unplanted reference of a committed case: computed once, shared, never written to."""
    c = WCASES[name]
    return wgrad_case_reference(*wgrad_operands(name, exact), c.taps, exact, plan_of(c))


def wgrad_planted(name, plant, exact=True):
    c = WCASES[name]
    return wgrad_case_reference(*wgrad_operands(name, exact), c.taps, exact, plan_of(c), plant)


def s2_wgrad_reference(x, dy, K):
    """fp64 conv2d_weight(stride=2, padding=K // 2).  x (B,H,W,C), dy (B,H/2,W/2,Co) -> (Co, C, K, K)."""
    return torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (dy.shape[3], x.shape[3], K, K),
                                       dy.double().permute(0, 3, 1, 2), stride=2, padding=K // 2)


def s2_wgrad_by_taps(x, dy, K, plant=None):
    """The stride-2 sum tap by tap -> (dw, S, n).  plant: one of S2_PLANTS."""
    if plant is not None and plant not in S2_PLANTS:
        raise NotExercised("not a plant of the stride-2 weight gradient")
    x, dy = x.double(), dy.double()
    B, H, W, Cc = x.shape
    Ho, Wo, Co = dy.shape[1], dy.shape[2], dy.shape[3]
    p = K // 2
    xr = x
    if plant == "phase_swapped":
        if K == 1:
            raise NotExercised("one phase plane")
        xr = C._swap_phases(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    if plant == "k1_wrong_phase":
        if K != 1:
            raise NotExercised("every phase plane is read")
        xr = _shift_cols(_shift_rows(x, 1), 1)    # phase (1, 1) in the place of (0, 0)
    pad = lambda t: F.pad(t, (0, 0, p, p + 1, p, p + 1))  # noqa: E731
    xp, xa = pad(xr), pad(x.abs())
    ones = pad(torch.ones(1, H, W, 1, dtype=torch.float64))
    dw = torch.zeros(Co, Cc, K, K, dtype=torch.float64)
    S = torch.zeros_like(dw)
    n = torch.zeros(K, K, dtype=torch.float64)
    for ky in range(K):
        for kx in range(K):
            win = lambda t: t[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]  # noqa: E731
            dw[:, :, ky, kx] = torch.einsum("byxo,byxc->oc", dy, win(xp))
            S[:, :, ky, kx] = torch.einsum("byxo,byxc->oc", dy.abs(), win(xa))
            n[ky, kx] = B * float(win(ones).sum())
    return dw, S, n


def s2_case_reference(x, dy, K, exact, plant=None):
    dw, S, n = s2_wgrad_by_taps(x, dy, K)
    if exact:
        assert_exact_precondition(x, dy)
    bound = wgrad_bound(S, n, exact)
    if plant is not None:
        dw = exercised(s2_wgrad_by_taps(x, dy, K, plant)[0], dw, bound, plant)
    return WRef(dw, S, n, bound)


@functools.lru_cache(maxsize=None)
def s2_ref(name, exact=True):
    return s2_case_reference(*s2_operands(name, exact), S2_BY_NAME[name].K, exact)


def expected_f32(ref64):
    """An exact case's fp64 value as the fp32 tensor the kernel must equal (the value IS an fp32 number)."""
    f = ref64.float()
    assert torch.equal(f.double(), ref64)
    return f


# ----------------------------------------------------------------------------------------------------------------------
# upsample + concat and its adjoint
# ----------------------------------------------------------------------------------------------------------------------
def coord_delta(n_in):
    """delta of the module docstring: the two fp32 roundings of r * Y."""
    return 2.1 * U32 * (n_in - 1)


def hat_matrix(n_in, up, align_corners=True):
    """(A, cand): A[Y, y] = the weight of low-res y in high-res Y, fp64; cand[Y, y] = |sY - y| < 1 + delta."""
    n_out = n_in * up
    if not align_corners:
        A = F.interpolate(torch.eye(n_in, dtype=torch.float64)[None], size=n_out, mode="linear", align_corners=False)[0].t()
        return A.contiguous(), A > 0
    i0, i1, f = C._axis64(n_in, n_out)
    A = torch.zeros(n_out, n_in, dtype=torch.float64)
    o = torch.arange(n_out)
    A[o, torch.from_numpy(i0)] += torch.from_numpy(1.0 - f)
    A[o, torch.from_numpy(i1)] += torch.from_numpy(f)
    s = torch.from_numpy(i0 + f).view(-1, 1)
    cand = (s - torch.arange(n_in, dtype=torch.float64).view(1, -1)).abs() < 1.0 + coord_delta(n_in)
    return A, cand


def _axis_f32(n_in, up):
    """The kernels' float32 coordinates of one axis: (r, i0, i1, l) with l = fl(s - i0) unquantised."""
    n_out = n_in * up
    r = C._ratio32(n_in, n_out)
    s = (r * np.arange(n_out).astype(np.float32)).astype(np.float32)
    i0 = s.astype(np.int64)
    return r, i0, i0 + (i0 < n_in - 1), (s - i0.astype(np.float32)).astype(np.float32)


def cat_f32(x, up):
    """upsample_cat_kernel's blend of bf16-valued x (B,H,W,C) in float32, operation by operation, NOT rounded to bf16:
    (1 - ly) ((1 - lx) a + lx b) + ly ((1 - lx) c + lx d)."""
    B, H, W, Ch = x.shape
    _, y0, y1, ly = _axis_f32(H, up)
    _, x0, x1, lx = _axis_f32(W, up)
    a, b, c, d = C._corners(x.float(), y0, y1, x0, x1)
    ly, lx = torch.from_numpy(ly).view(1, -1, 1, 1), torch.from_numpy(lx).view(1, 1, -1, 1)
    r = (1.0 - ly) * ((1.0 - lx) * a + lx * b) + ly * ((1.0 - lx) * c + lx * d)
    assert r.dtype == torch.float32
    return r


def _window_f32(n_in, up):
    """The adjoint kernels' candidate window and weights of one axis in float32: (lo (n_in), span, wgt (n_in, span),
    idx (n_in, span)): candidate i of low-res y is high-res lo[y] + i, weight 0 past the window's end."""
    n_out = n_in * up
    r, i0, _, l = _axis_f32(n_in, up)
    yv = np.arange(n_in)
    lo = np.maximum(0, np.floor((yv - 1).astype(np.float32) / r).astype(np.int64))
    hi = np.minimum(n_out - 1, np.ceil((yv + 1).astype(np.float32) / r).astype(np.int64))
    span = int((hi - lo).max()) + 1
    idx = lo[:, None] + np.arange(span)[None, :]
    live = idx <= hi[:, None]
    idc = np.minimum(idx, n_out - 1)
    c0, lf = i0[idc], l[idc]
    w = np.where(c0 == yv[:, None], np.float32(1) - lf,
                 np.where((c0 + 1 == yv[:, None]) & (c0 < n_in - 1), lf, np.float32(0))).astype(np.float32)
    return lo, span, np.where(live, w, np.float32(0)).astype(np.float32), idc


def adjoint_f32(g, c_off, Cx, up):
    """upsample_bwd_kernel (= the rows forms: the same sums in the same order) in float32: the candidate window from the
    fp32 divisions, wgt = fl(wy * wx), acc = fmaf(wgt, v, acc) over Y outer, X inner.  NOT rounded to bf16."""
    B, Hh, Wh, _ = g.shape
    H, W = Hh // up, Wh // up
    _, sy, wy, iy = _window_f32(H, up)
    _, sx, wx, ix = _window_f32(W, up)
    gs = g[..., c_off:c_off + Cx].float()
    acc = torch.zeros(B, H, W, Cx, dtype=torch.float32)
    wy, wx, iy, ix = torch.from_numpy(wy), torch.from_numpy(wx), torch.from_numpy(iy), torch.from_numpy(ix)
    for i in range(sy):
        rows = gs[:, iy[:, i]]                      # (B, H, Wh, Cx)
        for j in range(sx):
            wgt = (wy[:, i].view(H, 1) * wx[:, j].view(1, W)).view(1, H, W, 1)
            assert wgt.dtype == torch.float32
            v = rows[:, :, ix[:, j]]                # (B, H, W, Cx): candidate (i, j) of every low-res pixel
            acc = torch.where(wgt != 0, C._fma32(wgt.expand_as(acc), v, acc), acc)
    return acc


def adjoint_form(W, up, rows_switch=True):
    """The kernel lss_upsample_bwd_nhwc launches: "rows8", "rows12" or "walk"."""
    rx = C._ratio32(W, W * up)
    span = int(np.ceil(np.float32(2.0) / rx)) + 3
    if rows_switch and span <= 8:
        return "rows8"
    if rows_switch and span <= 12:
        return "rows12"
    return "walk"


@functools.lru_cache(maxsize=None)
def up_operands(name):
    """x (B,H,W,Cx), x2 (B,Hh,Wh,C2) | None, g (B,Hh,Wh,C2+Cx): fp32 tensors of bf16 values.  Exact cases: integers in
    [-3, 3], the sentinel in x2 and in the first C2 channels of g."""
    c = UP_BY_NAME[name]
    gen = _gen(name)
    Hh, Wh = c.H * c.up, c.W * c.up
    if c.exact:
        x = _ints((c.B, c.H, c.W, c.Cx), gen, 3)
        x2 = torch.full((c.B, Hh, Wh, c.C2), SENTINEL) if c.C2 else None
        g = torch.cat([torch.full((c.B, Hh, Wh, c.C2), SENTINEL), _ints((c.B, Hh, Wh, c.Cx), gen, 3)], 3)
    else:
        x = bf16_round(torch.randn(c.B, c.H, c.W, c.Cx, generator=gen))
        x2 = bf16_round(torch.randn(c.B, Hh, Wh, c.C2, generator=gen)) if c.C2 else None
        g = bf16_round(torch.randn(c.B, Hh, Wh, c.C2 + c.Cx, generator=gen))
    return x, x2, g


UpRef = collections.namedtuple("UpRef", "cat cat_bound dx dx_bound")


def up_reference(x, x2, g, up, exact, plant=None):
    """UpRef, fp64 and unrounded: cat (B,Hh,Wh,C2+Cx), dx (B,H,W,Cx) and their elementwise bounds (None for an exact
    case: the kernel must give `expected_bf16` of the value).  plant: one of UP_PLANTS, applied to dx."""
    if plant is not None and plant not in UP_PLANTS:
        raise NotExercised("not a plant of the upsample adjoint")
    B, H, W, Cx = x.shape
    C2 = 0 if x2 is None else x2.shape[3]
    Ay, cy = hat_matrix(H, up)
    Ax, cx = hat_matrix(W, up)
    v = torch.einsum("Yy,byxc,Xx->bYXc", Ay, x.double(), Ax)
    gs = g.double()[..., C2:C2 + Cx]
    dx = torch.einsum("Yy,bYXc,Xx->byxc", Ay, gs, Ax)
    if exact:
        assert up == 3 and H in (3, 11, 43) and W in (3, 11, 43)
        assert bool((x == x.round()).all()) and bool((g == g.round()).all()) and float(x.abs().max()) <= 3
        assert float(gs.abs().max()) <= 3
        for t in (v, dx, torch.einsum("Yy,bYXc,Xx->byxc", Ay, gs.abs(), Ax)):    # multiples of 2^-12 below 2^7
            assert bool((t * 4096 == (t * 4096).round()).all()) and float(t.abs().max()) < 128
        assert torch.equal(cat_f32(x, up).double(), v), "the concat's fp32 blend is not exact"
        assert torch.equal(adjoint_f32(g, C2, Cx, up).double(), dx), "the adjoint's fp32 sum is not exact"
        dv = E = None
    else:
        v2, rng, qmax = C.blend64(x.double(), up)
        assert float((v2 - v).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max()))
        dly, dlx = coord_delta(H), coord_delta(W)
        dv = (dly + dlx + 2 * U32) * rng + 10 * U32 * qmax
        ga = gs.abs()
        ncand = cy.double().sum(0).view(1, H, 1, 1) * cx.double().sum(0).view(1, 1, W, 1)
        E = torch.einsum("Yy,bYXc,Xx->byxc", cy.double(), ga, cx.double()) * (dly + dlx + 4 * U32) \
            + (ncand + 2) * U32 * torch.einsum("Yy,bYXc,Xx->byxc", Ay, ga, Ax)
    cat = v if x2 is None else torch.cat([x2.double(), v], 3)
    if exact:
        cat_bound = dx_bound = None
    else:
        cat_bound = bf16_out_bound(v, dv)
        if x2 is not None:
            cat_bound = torch.cat([torch.zeros_like(x2, dtype=torch.float64), cat_bound], 3)
        dx_bound = bf16_out_bound(dx, E)
    if plant is not None:
        py, px, gp = Ay, Ax, gs
        if plant == "adjoint_not_align_corners":
            if up == 1:
                raise NotExercised("both conventions are the identity")
            py, px = hat_matrix(H, up, False)[0], hat_matrix(W, up, False)[0]
        if plant == "adjoint_last_row_clamp":    # the last low-res row loses the weights l of the cell above it
            py = Ay.clone()
            y0 = torch.from_numpy(C._axis64(H, H * up)[0])
            py[y0 == H - 2, H - 1] = 0
        if plant == "adjoint_window_one_short":  # candidates end one before min(Hh - 1, ceil((y + 1) / r))
            py, px = Ay.clone(), Ax.clone()
            for A_, n_ in ((py, H), (px, W)):
                for yy in range(n_):
                    hi = min(n_ * up - 1, -(-(yy + 1) * (n_ * up - 1) // (n_ - 1)))
                    A_[hi, yy] = 0
        if plant == "c_off_ignored":
            if C2 == 0:
                raise NotExercised("no skip tensor: c_off = 0")
            gp = g.double()[..., :Cx]
        planted = torch.einsum("Yy,bYXc,Xx->byxc", py, gp, px)
        want = bf16_rn(dx) if exact else dx
        got = bf16_rn(planted) if exact else planted
        exercised(got, want, torch.zeros_like(dx) if exact else dx_bound, plant)
        dx = planted
    return UpRef(cat, cat_bound, dx, dx_bound)


@functools.lru_cache(maxsize=None)
def up_ref(name):
    c = UP_BY_NAME[name]
    return up_reference(*up_operands(name), c.up, c.exact)


def expected_bf16(ref64):
    """fp64 -> the bf16 tensor of its single rounding (round to nearest even)."""
    r = bf16_rn(ref64)
    out = r.float().bfloat16()
    assert torch.equal(out.double(), r)
    return out
