"""The helper of the K15 tests checked without a GPU (tests/txt_heads_ref.py): each reference IS the project's torch
modules (heads.BevPost, the embedders, cat, Linear, the predictors) in fp64 on every case; `check` rejects every planted
error on at least one case - every time the plant is exercised, but for the one rounding plant - and accepts the
unplanted simulation; no case is blind to every plant."""
import pytest
import torch

import txt_heads_ref as R

IDS = [c.name for c in R.CASES]
_cache = {}


def _heads(c, plant=None):
    key = (c.name, plant)
    if key not in _cache:
        if (c.name, "in") not in _cache:
            _cache[(c.name, "in")] = R.make_head_inputs(c)
        _cache[key] = R.ref_txt_heads(*_cache[(c.name, "in")], c.cams, c.ncams, plant=plant)
    return _cache[key]


def _post(c, plant=None):
    key = (c.name, "post", plant)
    if key not in _cache:
        if (c.name, "post_in") not in _cache:
            _cache[(c.name, "post_in")] = R.make_post_inputs(c)
        _cache[key] = R.ref_bev_post(_cache[(c.name, "post_in")][0], c.origin, c.crop, *_cache[(c.name, "post_in")][1:],
                                     plant=plant)
    return _cache[key]


@pytest.mark.parametrize("c", R.CASES + R.POST_EXTRA, ids=IDS + [c.name for c in R.POST_EXTRA])
def test_bev_post_reference_is_the_module(c):
    ref = _post(c)
    want = R.torch_bev_post(c, *_cache[(c.name, "post_in")])
    assert ref.y.shape == want.shape == (c.B, c.Cp, c.H, c.W) == (c.B, c.Cp) + R.post_out_size(*c.crop)
    assert float((ref.y - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert bool((ref.bound > 0).all()) and float(ref.bound.max()) < 1e-4   # a bound, and an fp32-sized one
    R.check(ref.y_sim, ref.y, ref.bound, "unplanted bev_post")


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_heads_reference_is_the_modules(c):
    ref = _heads(c)
    act, desc = R.torch_heads(c, *_cache[(c.name, "in")])
    assert ref.act.shape == act.shape == (c.B, c.n_act)
    assert ref.desc.shape == desc.shape == (c.B, c.n_desc_f + len(c.cams) - 1)
    for got, want in ((ref.act, act), (ref.desc, desc)):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    for b in (ref.bound_act, ref.bound_desc):
        assert bool((b > 0).all()) and float(b.max()) < 1e-2
    R.check(ref.act_sim, ref.act, ref.bound_act, "unplanted act")
    R.check(ref.desc_sim, ref.desc, ref.bound_desc, "unplanted desc")


def _rejected(c, plant):
    """Does `check` refuse what a kernel with the planted defect writes?  Raises NotExercised with the plant."""
    if plant in R.POST_PLANTS:
        ref, bad = _post(c), _post(c, plant)
        pairs = [(bad.y_sim, ref.y, ref.bound)]
    else:
        ref, bad = _heads(c), _heads(c, plant)
        pairs = [(bad.act_sim, ref.act, ref.bound_act), (bad.desc_sim, ref.desc, ref.bound_desc)]
    hit = False
    for got, want, bound in pairs:
        try:
            R.check(got, want, bound, plant)
        except AssertionError:
            hit = True
    return hit


@pytest.mark.parametrize("plant", R.PLANTS)
def test_every_plant_is_rejected(plant):
    """Rejected on at least one case; a plant that moves whole products or pixels is rejected on EVERY case that
    exercises it.  The rounding plant (half bf16 ulps of either sign) must show on pixel_1x1, where nothing averages."""
    rejected = 0
    for c in R.CASES:
        try:
            hit = _rejected(c, plant)
        except R.NotExercised:
            continue
        if plant != "embed_rounded_to_bf16" or c.name == "pixel_1x1":
            assert hit, (plant, c.name)
        rejected += hit
    assert rejected >= 1, plant


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_no_case_is_blind_to_every_plant(c):
    seen = 0
    for plant in R.PLANTS:
        try:
            _rejected(c, plant)
            seen += 1
        except R.NotExercised:
            pass
    assert seen >= 1, c.name


def test_cases_that_cannot_show_a_plant_say_so():
    one = R.BY_NAME["pixel_1x1"]
    for plant in ("tap_from_neighbour_image", "front_predictors_swapped"):
        with pytest.raises(R.NotExercised):
            _heads(one, plant)
    with pytest.raises(R.NotExercised):
        _heads(R.BY_NAME["production"], "padding_rows_enter_linear")
    for plant in ("side_uses_front_weights", "side_cameras_in_index_order"):
        with pytest.raises(R.NotExercised):
            _heads(R.BY_NAME["one_slot"], plant)
    with pytest.raises(R.NotExercised):
        _post(R.BY_NAME["tiles_5x7"], "conv_reads_outside_crop")
    with pytest.raises(ValueError):
        R.ref_txt_heads(*R.make_head_inputs(one), one.cams, one.ncams, plant="no_such_plant")
    with pytest.raises(ValueError):
        R.ref_bev_post(*R.make_post_inputs(one)[:1], one.origin, one.crop, *R.make_post_inputs(one)[1:], plant="nope")


def test_the_case_table_is_the_issues():
    assert [(c.name, c.B, c.H, c.W) for c in R.CASES] == [("production", 2, 8, 22), ("partial_3x5", 3, 3, 5),
                                                          ("tiles_5x7", 2, 5, 7), ("pixel_1x1", 2, 1, 1),
                                                          ("one_slot", 1, 3, 5)]
    p = R.BY_NAME["production"]
    assert (p.map, p.origin, p.crop, p.Cb, p.Cp, p.cams) == ((200, 200), (60, 56), (80, 88), 4, 8, (1, 0, 3, 2, 5))
    assert [(c.H * c.W) % R.TILE for c in R.CASES] == [0, 15, 3, 1, 15]
    assert all(R.post_out_size(*c.crop) == (c.H, c.W) for c in R.CASES + R.POST_EXTRA)
    assert R.BY_NAME["one_slot"].ncams == 2 and R.BY_NAME["one_slot"].cams == (1,)
    assert torch.equal(R.bf16(R.make_head_inputs(R.BY_NAME["pixel_1x1"])[0]), R.make_head_inputs(R.BY_NAME["pixel_1x1"])[0])
