"""`augmentate` split into `draw_augmentation` (every random decision, as a plan) and `apply_augmentation` (no draws): the
split takes the same decisions from the same generator states and gives the same arrays, and the plan packs into the record
the device kernel reads."""
import os
import random

import numpy as np
import pytest

from modular_semantic_segmentation_amd import _lib
from modular_semantic_segmentation_amd.datasets import augmentation as aug
from modular_semantic_segmentation_amd.datasets import device_augmentation as dev

CONFIG = {'crop': [1, 24], 'scale': [.7, .7, 1.5], 'rotate': [.6, -13, 13], 'shear': [.5, .01, .1], 'vflip': .6, 'hflip': .6,
          'gamma': [.5, .3, 1.2], 'contrast': [.5, .5, 1.5], 'brightness': [.5, -40, 40], 'label_flip': [3, 4],
          'label_merge': [1, 2]}
H, W = 40, 56


def make_blob(seed):
    rng = np.random.default_rng(1000 + seed)
    depth = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    depth[0, 0], depth[-1, -1] = 65535, 0
    return {'rgb': rng.integers(0, 256, (H, W, 3)).astype(np.uint8), 'depth': depth,
            'labels': rng.integers(0, 12, (H, W)).astype(np.int32)}


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)


SEEDS = list(range(20))


@pytest.mark.parametrize('seed', SEEDS)
def test_draw_then_apply_is_augmentate(seed):
    seed_all(seed)
    want = aug.augmentate(make_blob(seed), **CONFIG)
    states = random.getstate(), np.random.get_state()
    seed_all(seed)
    plan = aug.draw_augmentation(H, W, **CONFIG)
    assert random.getstate() == states[0]
    got_state = np.random.get_state()
    assert got_state[0] == states[1][0] and np.array_equal(got_state[1], states[1][1]) and got_state[2:] == states[1][2:]
    got = aug.apply_augmentation(make_blob(seed), plan)
    assert random.getstate() == states[0]                       # applying draws nothing
    assert sorted(got) == sorted(want)
    for m in want:
        assert got[m].dtype == want[m].dtype and np.array_equal(got[m], want[m]), m
    assert plan['size'] == want['rgb'].shape[:2] == (24, 24)


def test_draw_raises_where_augmentate_raises():
    """A crop larger than the image fails in the crop draw, in both."""
    config = dict(CONFIG, crop=[1, 48], scale=False)
    for call in (lambda: aug.augmentate(make_blob(0), **config), lambda: aug.draw_augmentation(H, W, **config)):
        seed_all(0)
        with pytest.raises(ValueError):
            call()


def test_draws_without_rgb_skip_the_photometric_ones():
    for seed in SEEDS[:5]:
        blob = {m: v for m, v in make_blob(seed).items() if m != 'rgb'}
        seed_all(seed)
        want = aug.augmentate(dict(blob), **CONFIG)
        state = np.random.get_state()[1].copy()
        seed_all(seed)
        plan = aug.draw_augmentation(H, W, has_rgb=False, **CONFIG)
        assert np.array_equal(np.random.get_state()[1], state)
        assert plan['contrast'] is None and plan['brightness'] is None and plan['gamma'] is None
        got = aug.apply_augmentation({m: v for m, v in make_blob(seed).items() if m != 'rgb'}, plan)
        assert all(np.array_equal(got[m], want[m]) for m in want)


@pytest.mark.parametrize('seed', SEEDS)
def test_composed_table_is_the_three_steps_in_turn(seed):
    seed_all(seed)
    plan = aug.draw_augmentation(H, W, **CONFIG)
    values = np.arange(256).astype(np.uint8)
    if plan['contrast'] is not None:                             # the host's formulas, restated
        values = np.clip(np.rint(128.0 + plan['contrast'] * (values.astype(np.float64) - 128.0)), 0, 255).astype(np.uint8)
    if plan['brightness'] is not None:
        values = np.clip(np.rint(values.astype(np.float64) + plan['brightness']), 0, 255).astype(np.uint8)
    if plan['gamma'] is not None:
        values = (((np.arange(256) / 255.0) ** (1 / plan['gamma'])) * 255).astype('uint8')[values]
    table = aug.photometric_table(plan)
    assert table.dtype == np.uint8 and np.array_equal(table, values)
    # and it is what apply_augmentation does to an image: a ramp through the chain
    ramp = {'rgb': np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (4, 256, 3)).copy()}
    only = dict(plan, scale=None, rotate=None, shear=None, crop=None, hflip=False, vflip=False, label_flip=None,
                label_merge=None)
    assert np.array_equal(aug.apply_augmentation(ramp, only)['rgb'][0, :, 0], table)


def test_every_table_kind_occurs():
    kinds = set()
    for seed in SEEDS:
        seed_all(seed)
        plan = aug.draw_augmentation(H, W, **CONFIG)
        kinds.add(tuple(plan[k] is not None for k in ('contrast', 'brightness', 'gamma')))
    assert {k[0] for k in kinds} == {k[1] for k in kinds} == {k[2] for k in kinds} == {False, True}


def test_packed_plan_is_the_library_record():
    seed_all(SEEDS[0])
    plans = [aug.draw_augmentation(H, W, **CONFIG) for _ in range(3)]
    records = dev.pack_plans(plans, H, W)
    assert records.shape == (3,) and records.dtype == dev.PLAN_DTYPE
    names = list(dev.PLAN_DTYPE.names)
    assert names[:2] == ['scale_ry', 'scale_rx'] and names[-1] == 'merge_drop'
    assert dev.PLAN_DTYPE.itemsize == 14 * 8 + 16 * 4            # no padding: doubles first
    assert dev.pack_tables(plans).shape == (3, 256)
    for rec, plan in zip(records, plans):
        assert bool(rec['stages'] & dev.STAGE_BITS['XVA_ROTATE']) == (plan['rotate'] is not None)
        assert rec['crop_size'] == 24 and (rec['flip_from'], rec['flip_to']) == tuple(plan['label_flip'])
    if os.path.exists(_lib.LIB_PATH):
        assert dev.PLAN_DTYPE.itemsize == _lib.lib().xv_augment_plan_bytes()
    with pytest.raises(ValueError, match='crop'):
        dev.pack_plans([dict(plans[0], crop=None)], H, W)
