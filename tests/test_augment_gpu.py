"""On-device training augmentation (csrc/augment.hip, ops.augment_batch, datasets/device_augmentation.py) against the host
chain it restates: `apply_augmentation` + `crop_multiple` + the float cast of `DataBaseclass._load_sample`.  Every comparison
is np.array_equal: the kernel computes in float64 in numpy's operation order, without contraction."""
import ctypes
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from modular_semantic_segmentation_amd.datasets import augmentation as aug
from modular_semantic_segmentation_amd.datasets import device_augmentation as dev
from oracle import fcn_oracle as fo

DEV = 'cuda:0'
M, H, W = 5, 40, 56
CONFIG = {'crop': [1, 24], 'scale': [.7, .7, 1.5], 'rotate': [.6, -13, 13], 'shear': [.5, .01, .1], 'vflip': .6, 'hflip': .6,
          'gamma': [.5, .3, 1.2], 'contrast': [.5, .5, 1.5], 'brightness': [.5, -40, 40], 'label_flip': [3, 4],
          'label_merge': [1, 2]}
GEOMETRIC = ('scale', 'rotate', 'shear', 'hflip', 'vflip')


@pytest.fixture(scope='module')
def gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _host_pool():
    rng = np.random.default_rng(7)
    depth = rng.integers(1, 65536, (M, H, W)).astype(np.uint16)
    depth[:, 0, 0], depth[:, -1, -1] = 65535, 1
    return {'rgb': rng.integers(0, 256, (M, H, W, 3)).astype(np.uint8), 'depth': depth,
            'labels': rng.integers(0, 12, (M, H, W)).astype(np.int32)}


POOL = _host_pool()


@pytest.fixture(scope='module')
def pool(gpu):
    return {m: torch.from_numpy(v).to(DEV) for m, v in POOL.items()}


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)


def draw(config, seed, count):
    """`count` plans from one seed, or None where the host chain itself refuses (a rotation that leaves less than the crop)."""
    seed_all(seed)
    try:
        return [aug.draw_augmentation(H, W, **config) for _ in range(count)]
    except ValueError:
        return None


def stages_of(plan):
    return frozenset(k for k in GEOMETRIC if plan[k])


def host_sample(item, plan):
    """What the host stream makes of pool item `item` under `plan` (DataBaseclass._load_sample)."""
    out = aug.apply_augmentation({m: v[item].copy() for m, v in POOL.items()}, plan)
    out['depth'] = out['depth'][:, :, None]
    return {m: np.asarray(aug.crop_multiple(out[m])).astype('int32' if m == 'labels' else 'float32') for m in out}


def check_batch(pool, plans, index):
    from modular_semantic_segmentation_amd import ops
    index = np.asarray(index, np.int32)
    rgb, depth, labels = ops.augment_batch(pool, index, dev.pack_plans(plans, H, W), dev.pack_tables(plans))
    got = {'rgb': rgb.cpu().numpy(), 'depth': depth.cpu().numpy(), 'labels': labels.cpu().numpy()}
    size = plans[0]['crop']['size'] // 16 * 16
    assert got['rgb'].shape == (len(index), size, size, 3) and got['rgb'].dtype == np.float32
    assert got['depth'].shape == (len(index), size, size, 1) and got['depth'].dtype == np.float32
    assert got['labels'].shape == (len(index), size, size) and got['labels'].dtype == np.int32
    for n, (item, plan) in enumerate(zip(index, plans)):
        want = host_sample(item, plan)
        for m in want:
            assert np.array_equal(got[m][n], want[m]), (m, n, sorted(stages_of(plan)))
    return got


def _chosen_batches():
    """Seeds whose three images take three different stage subsets, picked until every stage has occurred alone and together
    with others.  -> [(seed, plans)], the stage subsets seen"""
    need = {(k, alone) for k in GEOMETRIC for alone in (True, False)}
    batches, seen = [], set()
    for seed in range(4000):
        plans = draw(CONFIG, seed, 3)
        if plans is None:
            continue
        subsets = [stages_of(p) for p in plans]
        new = {(k, len(s) == 1) for s in subsets for k in s} & need
        if len(set(subsets)) == 3 and new:
            batches.append((seed, plans))
            seen.update(subsets)
            need -= new
        if not need:
            break
    return batches, seen


BATCHES, SEEN = _chosen_batches()


def test_chosen_batches_cover_every_stage_alone_and_combined():
    assert 1 <= len(BATCHES) <= 12
    for k in GEOMETRIC:
        assert frozenset([k]) in SEEN, k
        assert any(k in s and len(s) > 1 for s in SEEN), k
    for _, plans in BATCHES:
        assert len({stages_of(p) for p in plans}) == 3
    every = [p for _, plans in BATCHES for p in plans]
    for k in ('contrast', 'brightness', 'gamma'):
        assert any(p[k] is not None for p in every) and any(p[k] is None for p in every), k
    assert {p['label_flip'] for p in every} == {(3, 4), (4, 3)}


@pytest.mark.parametrize('seed,plans', BATCHES, ids=[str(s) for s, _ in BATCHES])
def test_batch_equals_host_chain(pool, seed, plans):
    check_batch(pool, plans, [(seed + i) % M for i in range(3)])


@pytest.mark.parametrize('crop', [16, 24, 32])
def test_crop_sizes(pool, crop):
    """crop 16 and 24 both give 16 x 16 (24 is cut down by crop_multiple); 32 spans more than one tile per row"""
    config = dict(CONFIG, crop=[1, crop])
    seed = next(s for s in range(200) if draw(config, s, 3) is not None and
                any(len(stages_of(p)) >= 3 for p in draw(config, s, 3)))
    got = check_batch(pool, draw(config, seed, 3), [0, 2, 3])
    assert got['labels'].shape[1] == crop // 16 * 16


def _edge(pool, config, predicate, index=(1,), count=1):
    config = dict({'crop': [1, 16]}, **config)
    for seed in range(400):
        plans = draw(config, seed, count)
        if plans is not None and predicate(plans):
            return plans, check_batch(pool, plans, list(index))
    raise AssertionError('no seed gives the case')


def test_edge_scale_below_one(pool):
    plans, _ = _edge(pool, {'scale': [1, .5, .5]}, lambda p: True)
    assert plans[0]['scale']['size'] == (20, 28)


def test_edge_scale_above_one(pool):
    plans, _ = _edge(pool, {'scale': [1, 1.5, 1.5]}, lambda p: True)
    assert plans[0]['scale']['size'] == (60, 84)


def test_edge_rotation_by_zero(pool):
    plans, _ = _edge(pool, {'rotate': [1, 0, 1]}, lambda p: True)
    assert plans[0]['rotate']['degrees'] == 0 and plans[0]['rotate']['canvas'] == (H, W)


def test_edge_rotation_by_a_negative_angle(pool):
    plans, _ = _edge(pool, {'rotate': [1, -13, -12]}, lambda p: True)
    assert plans[0]['rotate']['degrees'] == -13


def test_edge_rotation_canvas_exceeds_source(pool):
    plans, _ = _edge(pool, {'rotate': [1, 12, 13]}, lambda p: True)
    canvas = plans[0]['rotate']['canvas']
    assert canvas[0] > H and canvas[1] > W


def test_edge_shear_border_inside_the_crop(pool):
    """a 16-degree shear moves the top and bottom rows by 5.7 pixels: with a 32-pixel crop at the left edge the zero wedge is
    inside the window (depth in the pool is never 0, so a zero there is border)"""
    plans, got = _edge(pool, {'crop': [1, 32], 'shear': [1, .3, .31]}, lambda p: p[0]['crop']['left'] == 0)
    assert abs(plans[0]['shear']['degrees']) == 16
    border = got['depth'][0, ..., 0] == 0
    assert border.any() and not border.all()


def test_edge_both_flips(pool):
    plans, _ = _edge(pool, {'hflip': 1, 'vflip': 1}, lambda p: p[0]['hflip'] and p[0]['vflip'])
    assert stages_of(plans[0]) == {'hflip', 'vflip'}


def test_edge_repeated_index_and_last_pool_image(pool):
    got = _edge(pool, CONFIG, lambda p: True, index=(M - 1, M - 1, 1), count=3)[1]
    assert got['rgb'].shape[0] == 3


def test_edge_single_image(pool):
    got = _edge(pool, CONFIG, lambda p: len(stages_of(p[0])) >= 2, index=(M - 1,))[1]
    assert got['rgb'].shape[0] == 1


# ---- ABI refusals ---------------------------------------------------------------------------------------------------------

def _raw_call(pool, records, index, size, null=None, tables=None):
    """xv_augment_batch on sentinel-filled outputs -> (return code, outputs untouched?)"""
    from modular_semantic_segmentation_amd import _lib
    n = len(index)
    index = np.ascontiguousarray(index, np.int32)
    tables = np.tile(np.arange(256, dtype=np.uint8), (n, 1)) if tables is None else tables
    d_index, d_tables = torch.from_numpy(index).to(DEV), torch.from_numpy(tables).to(DEV)
    d_plans = torch.from_numpy(records.view(np.uint8).reshape(-1).copy()).to(DEV)
    side = max(size, 16)
    outs = [torch.full((n, side, side, 3), -7.0, device=DEV), torch.full((n, side, side, 1), -7.0, device=DEV),
            torch.full((n, side, side), -7, dtype=torch.int32, device=DEV)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    args = {'rgb': p(pool['rgb']), 'depth': p(pool['depth']), 'labels': p(pool['labels']), 'index': p(d_index),
            'index_host': index.ctypes.data_as(ctypes.c_void_p), 'plans': p(d_plans),
            'plans_host': records.ctypes.data_as(ctypes.c_void_p), 'luts': p(d_tables), 'out_rgb': p(outs[0]),
            'out_depth': p(outs[1]), 'out_labels': p(outs[2])}
    if null is not None:
        args[null] = None
    rc = _lib.lib().xv_augment_batch(args['rgb'], args['depth'], args['labels'], M, H, W, args['index'], args['index_host'],
                                     args['plans'], args['plans_host'], args['luts'], n, size, args['out_rgb'],
                                     args['out_depth'], args['out_labels'],
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, all(bool((o == -7).all()) for o in outs)


def _plain_records(n=2):
    """crop-only plans: the 16 x 16 window at (3, 5)"""
    plan = dict(draw({'crop': [1, 16]}, 0, 1)[0])
    plan['crop'] = {'top': 3, 'left': 5, 'size': 16}
    return dev.pack_plans([plan] * n, H, W)


def test_abi_accepts_the_plain_call(pool):
    rc, untouched = _raw_call(pool, _plain_records(), [0, 4], 16)
    assert rc == 0 and not untouched


@pytest.mark.parametrize('null', ['rgb', 'depth', 'labels', 'index', 'index_host', 'plans', 'plans_host', 'luts', 'out_rgb',
                                  'out_depth', 'out_labels'])
def test_abi_refuses_null_pointers(pool, null):
    assert _raw_call(pool, _plain_records(), [0, 4], 16, null=null) == (-1, True)


@pytest.mark.parametrize('size', [0, -16, 8, 24])
def test_abi_refuses_sizes_that_are_no_positive_multiple_of_16(pool, size):
    records = _plain_records()
    records['crop_size'] = 24
    assert _raw_call(pool, records, [0, 4], size) == (-1, True)


@pytest.mark.parametrize('index', [[0, M], [-1, 0]])
def test_abi_refuses_an_index_outside_the_pool(pool, index):
    from modular_semantic_segmentation_amd import _lib, ops
    assert _raw_call(pool, _plain_records(), index, 16) == (-1, True)
    with pytest.raises(_lib.XvError, match='XV_EINVAL'):
        ops.augment_batch(pool, np.asarray(index, np.int32), _plain_records(), np.zeros((2, 256), np.uint8))


@pytest.mark.parametrize('member,value', [('crop_top', H - 15), ('crop_left', W - 15), ('crop_top', -1), ('crop_left', -1),
                                          ('crop_size', 15), ('rot_h', H - 1), ('scale_w', W + 1), ('stages', 128)])
def test_abi_refuses_a_plan_whose_window_leaves_its_image(pool, member, value):
    records = _plain_records()
    records[member][1] = value
    assert _raw_call(pool, records, [0, 4], 16) == (-1, True)


def test_abi_refuses_a_rotated_plan_whose_crop_leaves_the_inscribed_rectangle(pool):
    plans = next(p for p in (draw({'crop': [1, 16], 'rotate': [1, 12, 13]}, s, 1) for s in range(50)) if p is not None)
    records = dev.pack_plans(plans, H, W)
    assert _raw_call(pool, records, [2], 16)[0] == 0
    records['crop_left'] = records['rot_w'] - 15                     # inside the canvas, outside the cut
    assert records['crop_left'][0] + 16 <= records['canvas_w'][0]
    assert _raw_call(pool, records, [2], 16) == (-1, True)


# ---- DeviceTrainset -----------------------------------------------------------------------------------------------------------

def _stream_seed(batchsize, batches):
    count = batchsize * batches
    return next(s for s in range(200) if draw(CONFIG, s, count) is not None and
                len({stages_of(p) for p in draw(CONFIG, s, count)}) >= min(3, count))


def test_device_trainset_yields_the_host_stream(gpu):
    trainset = dev.DeviceTrainset(POOL, CONFIG, DEV)
    assert len(trainset) == M
    seed = _stream_seed(2, 3)
    items = [0, 1, 2, 3, 4, 0]                                        # the wrap is crossed in the third batch
    seed_all(seed)
    want = []
    for item in items:                                                # the host stream: one augmentate per item, in order
        blob = aug.augmentate({m: v[item].copy() for m, v in POOL.items()}, **CONFIG)
        blob['depth'] = blob['depth'][:, :, None]
        want.append({m: np.asarray(aug.crop_multiple(blob[m])).astype('int32' if m == 'labels' else 'float32')
                     for m in blob})
    host_state = random.getstate()
    seed_all(seed)
    batches = trainset.training_batches(2)
    for b in range(3):
        batch = next(batches)
        assert sorted(batch) == ['depth', 'labels', 'rgb'] and all(t.is_cuda for t in batch.values())
        for m, t in batch.items():
            assert np.array_equal(t.cpu().numpy(), np.stack([want[2 * b][m], want[2 * b + 1][m]])), (m, b)
    assert random.getstate() == host_state


def test_device_trainset_takes_lists_and_resident_tensors(pool):
    seed = _stream_seed(2, 1)
    outs = []
    for source in (POOL, {m: list(v) for m, v in POOL.items()}, pool, dict(POOL, depth=POOL['depth'][..., None])):
        seed_all(seed)
        outs.append(next(dev.DeviceTrainset(source, CONFIG, DEV).training_batches(2)))
    for other in outs[1:]:
        assert all(torch.equal(outs[0][m], other[m]) for m in outs[0])


def test_device_trainset_refusals(gpu):
    with pytest.raises(ValueError, match='crop'):
        dev.DeviceTrainset(POOL, dict(CONFIG, crop=False), DEV)
    with pytest.raises(ValueError, match='probability'):
        dev.DeviceTrainset(POOL, dict(CONFIG, crop=[.5, 24]), DEV)
    ragged = {m: list(v) for m, v in POOL.items()}
    ragged['rgb'][2] = ragged['rgb'][2][:-1]
    with pytest.raises(ValueError, match='one size'):
        dev.DeviceTrainset(ragged, CONFIG, DEV)
    with pytest.raises(ValueError, match='one size'):
        dev.DeviceTrainset(dict(POOL, labels=POOL['labels'][:, :-1]), CONFIG, DEV)
    with pytest.raises(ValueError, match='raw'):
        dev.DeviceTrainset(dict(POOL, depth=POOL['depth'].astype(np.float32)), CONFIG, DEV)


# ---- fit() through the hook ----------------------------------------------------------------------------------------------------

def _fcn(tmp_path, path):
    from modular_semantic_segmentation_amd import get_model
    desc = ({'rgb': 'float32', 'labels': 'int32'}, {'rgb': (None, None, 3), 'labels': (None, None)}, 12)
    net = get_model('fcn')('rgb', desc, 'rgb', output_dir=str(tmp_path), num_units=64, batch_normalization=False,
                           batchsize=2, learning_rate=1e-3, trainer='adam')
    net.import_weights(path, warnings=False)
    losses = []
    step = net._train_batch
    net._train_batch = lambda batch: losses.append(step(batch)) or losses[-1]
    return net, losses


def test_fit_takes_device_batches_through_the_hook(gpu, tmp_path):
    """Two steps from a DeviceTrainset and two steps from the same two batches as a dict of arrays, from the same weights: the
    trainer is bitwise reproducible run to run, so the losses and the exported weights are equal."""
    w = fo.init_fcn_weights('rgb', 3, 64, 12, seed=1, bias_scale=0.02)
    w['rgb/conv1_1/kernel'] *= 0.02
    path = str(tmp_path / 'w.npz')
    np.savez(path, **w)
    seed = _stream_seed(2, 2)

    trainset = dev.DeviceTrainset(POOL, CONFIG, DEV)
    calls = []
    batches_of = trainset.training_batches
    trainset.training_batches = lambda batchsize: calls.append(batchsize) or batches_of(batchsize)
    net, losses = _fcn(tmp_path / 'a', path)
    seed_all(seed)
    net.fit(trainset, 2, output=False)
    assert calls == [2] and len(losses) == 2
    from_device = dict(np.load(net.export_weights()))

    seed_all(seed)
    stream = dev.DeviceTrainset(POOL, CONFIG, DEV).training_batches(2)
    two = [next(stream), next(stream)]
    data = {m: np.concatenate([b[m].cpu().numpy() for b in two]) for m in two[0]}
    assert data['rgb'].shape == (4, 16, 16, 3)

    class Spy(dict):                                                  # a plain dict takes the old path
        def __getattr__(self, name):
            if name == 'training_batches':
                touched.append(name)
            raise AttributeError(name)
    touched = []
    other, other_losses = _fcn(tmp_path / 'b', path)
    other.fit(Spy(data), 2, output=False)
    assert touched == ['training_batches']                            # asked for, absent: the existing code ran
    assert other_losses[0] == losses[0]
    assert other_losses == losses
    from_arrays = dict(np.load(other.export_weights()))
    assert sorted(from_arrays) == sorted(from_device)
    for name in from_device:
        assert np.array_equal(from_device[name], from_arrays[name]), name
    assert any(not np.array_equal(from_device[k], w[k]) for k in w)   # and the steps did move the weights


# ---- the readers --------------------------------------------------------------------------------------------------------------

READER_AUGMENTATION = {'crop': [1, 16], 'scale': [.5, .7, 1.5], 'vflip': .3, 'hflip': False, 'gamma': [.4, .3, 1.2],
                       'rotate': [.4, -13, 13], 'shear': [.3, .01, .1], 'contrast': [.3, .5, 1.5], 'brightness': [.2, -40, 40]}


@pytest.mark.parametrize('reader', ['synthia', 'cityscapes'])
def test_get_device_trainset_yields_the_readers_own_stream(gpu, tmp_path, reader):
    """36 x 52 miniature trees (tests/dataset_fixtures.py): the first batches of `get_device_trainset` are the first samples of
    `get_trainset()` from the same seed, stacked"""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import dataset_fixtures as fx
    if reader == 'synthia':
        from modular_semantic_segmentation_amd.datasets.synthia_cityscapes import SynthiaCityscapes
        fx.build_synthia_tree(str(tmp_path))
        data = SynthiaCityscapes(base_path=str(tmp_path), augmentation=READER_AUGMENTATION)
    else:
        from modular_semantic_segmentation_amd.datasets.cityscapes import Cityscapes
        fx.build_cityscapes_tree(str(tmp_path))
        data = Cityscapes(base_path=str(tmp_path), augmentation=READER_AUGMENTATION)
    seed_all(0)
    want = []
    for sample in data.get_trainset():
        want.append(sample)
        if len(want) == 4:
            break
    trainset = data.get_device_trainset(DEV, num_items=4)
    assert len(trainset) == 4 and (trainset.height, trainset.width) == fx.IMAGE_HW
    seed_all(0)
    batches = trainset.training_batches(2)
    for b in range(2):
        batch = next(batches)
        for m in ('rgb', 'depth', 'labels'):
            got = batch[m].cpu().numpy()
            assert got.dtype == want[0][m].dtype
            assert np.array_equal(got, np.stack([want[2 * b][m], want[2 * b + 1][m]])), (m, b)
