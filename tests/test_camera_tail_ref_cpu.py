"""The reference of the K14 tests checked without a GPU (tests/camera_tail_ref.py): it IS the project's modules run in
double, it reproduces what the reference's own classes gave (tests/golden/g14_camera_branch.npz), the inputs of the GPU
tests are well conditioned (fp32 library arithmetic stays 4x inside the GPU test's bound), and a wrong GELU cannot pass
at that bound."""
import copy

import pytest
import torch

import camera_tail_ref as R

GPU_BOUND = 1e-5  # what tests/test_camera_tail_gpu.py grants the kernel


def _double(mods):
    out = copy.copy(mods)
    for k in ("camera_transformer", "bev_fusion", "unified_predictor"):
        m = getattr(mods, k)
        setattr(out, k, None if m is None else copy.deepcopy(m).double())
    return out


@pytest.mark.parametrize("n", R.NS)
@pytest.mark.parametrize("cam,fus", R.STAGES)
def test_reference_is_the_module_composition_in_double(n, cam, fus):
    mods = R.make_modules(n, 300 + n, cam, fus)
    tokens, bev = R.make_inputs(2, n, 17 + n)
    with torch.no_grad():
        want = R.library(_double(mods), tokens.double(), bev.double())
        got = R.tail(tokens, R.params_of(mods), bev)
    for g, w in zip(got, want):
        assert R.errors(g, w)[0] <= 1e-13, (n, cam, fus, R.errors(g, w))


def test_reference_reproduces_the_reference_classes(golden):
    """Fed g14's golden tokens and the regenerated BEV map it gives g14's action / description, within the bound
    `test_cpu_composition_reproduces_the_reference` grants the fp32 composition."""
    g = golden("g14_camera_branch")
    for name in ("a", "b"):
        mods, tokens, bev, action, description = R.g14_case(g, name)
        got = R.tail(tokens, R.params_of(mods), bev)
        for t, want in zip(got, (action, description)):
            assert R.errors(t, want)[0] <= 1e-5, (name, R.errors(t, want))


def _inputs(golden):
    for c in R.CASES:
        B, n, cam, fus, seed = c
        yield (R.case_id(c), R.make_modules(n, seed, cam, fus)) + R.make_inputs(B, n, seed + 1)
    g = golden("g14_camera_branch")
    for name in ("a", "b"):
        mods, tokens, bev, _, _ = R.g14_case(g, name)
        yield "g14_" + name, mods, tokens, bev.float()


def test_gpu_inputs_are_well_conditioned(golden):
    """The fp32 library composition on the CPU stays within 2.5e-6 of the fp64 reference on every input the GPU tests
    use, so their 1e-5 bound is at least 4x fp32's own error."""
    worst = 0.0
    for tag, mods, tokens, bev in _inputs(golden):
        with torch.no_grad():
            lib = R.library(mods, tokens, bev)
        want = R.tail(tokens, R.params_of(mods), bev)
        for t, w in zip(lib, want):
            e = R.errors(t, w)[0]
            worst = max(worst, e)
            assert e <= 2.5e-6, (tag, e)
    print("worst fp32 library error over the GPU tests' inputs: %.2e" % worst)
    assert 4 * worst <= GPU_BOUND


def test_tanh_gelu_is_separated_from_the_bound(golden):
    """The tanh approximation instead of erf moves the outputs by more than 1e-4: a wrong formula cannot pass at 1e-5."""
    g = golden("g14_camera_branch")
    for name in ("a", "b"):
        mods, tokens, bev, _, _ = R.g14_case(g, name)
        p = R.params_of(mods)
        want = R.tail(tokens, p, bev)
        wrong = R.tail(tokens, p, bev, tanh_gelu=True)
        for t, w in zip(wrong, want):
            assert R.errors(t, w)[0] > 1e-4, (name, R.errors(t, w))
