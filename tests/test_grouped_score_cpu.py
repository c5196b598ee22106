"""Host side of scoring by group: the bootstrap of a measure over per-image confusion matrices against a plain loop, the shared
measures helper, the per-sequence evaluation on a stub network, the key -> id mapping, and the new declarations in the ABI."""
import os
import re

import numpy as np
import pytest

from modular_semantic_segmentation_amd import _lib, base_model, experiments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 5


def _per_image(n, seed, empty_class=True):
    rng = np.random.default_rng(seed)
    cms = rng.integers(0, 50, (n, C, C)).astype(np.float64)
    if empty_class:
        cms[:, 3, :] = 0
        cms[:, :, 3] = 0                 # class 3 is never a label and never predicted: its IoU is NaN
    return cms


def _loop_samples(cms_list, measure, num_resamples, seed):
    """the same draws of numpy.random.RandomState(seed), one resample at a time, matrices summed image by image"""
    rng = np.random.RandomState(seed)
    n = len(cms_list[0])
    out = [[] for _ in cms_list]
    for _ in range(num_resamples):
        times = rng.multinomial(n, np.full(n, 1.0 / n))
        for dst, cms in zip(out, cms_list):
            total = np.zeros((C, C))
            for i in range(n):
                for _ in range(times[i]):
                    total += cms[i]
            dst.append(base_model.score_measures(total)[measure])
    return [np.array(o) for o in out]


@pytest.mark.parametrize('measure', ['mean_IoU', 'total_accuracy', 'mean_F1'])
def test_bootstrap_measure_equals_a_plain_loop(measure):
    cms = _per_image(7, 1)
    got = experiments.bootstrap_measure(cms, measure=measure, num_resamples=40, seed=3, interval=0.9)
    ref, = _loop_samples([cms], measure, 40, 3)
    assert got['samples'].dtype == np.float64 and np.array_equal(got['samples'], ref)
    assert got['value'] == base_model.score_measures(cms.sum(0))[measure]
    assert (got['low'], got['high']) == pytest.approx(tuple(np.percentile(ref, [5.0, 95.0])), rel=1e-12)
    assert got['low'] <= got['high'] and ref.min() <= got['low'] and got['high'] <= ref.max()
    # the seed fixes the draws
    assert np.array_equal(experiments.bootstrap_measure(cms, measure=measure, num_resamples=40, seed=3)['samples'], ref)
    assert not np.array_equal(experiments.bootstrap_measure(cms, measure=measure, num_resamples=40, seed=4)['samples'], ref)
    # what score_groups(..., 'image') returns is taken as it is
    keyed = {i: (base_model.score_measures(cm), cm) for i, cm in enumerate(cms)}
    assert np.array_equal(experiments.bootstrap_measure(keyed, measure=measure, num_resamples=40, seed=3)['samples'], ref)


def test_paired_bootstrap_equals_a_plain_loop_on_shared_draws():
    a, b = _per_image(6, 2), _per_image(6, 5)
    got = experiments.paired_bootstrap(a, b, num_resamples=50, seed=11)
    ref_a, ref_b = _loop_samples([a, b], 'mean_IoU', 50, 11)
    assert np.array_equal(got['samples'], ref_a - ref_b)
    assert got['fraction_a_better'] == np.mean(ref_a > ref_b)
    assert got['value'] == base_model.score_measures(a.sum(0))['mean_IoU'] - base_model.score_measures(b.sum(0))['mean_IoU']
    assert (got['low'], got['high']) == pytest.approx(tuple(np.percentile(ref_a - ref_b, [2.5, 97.5])), rel=1e-12)
    # both methods see the same resampled images: each side alone is bootstrap_measure with that seed
    assert np.array_equal(experiments.bootstrap_measure(a, num_resamples=50, seed=11)['samples'], ref_a)
    same = experiments.paired_bootstrap(a, a.copy(), num_resamples=50, seed=11)
    assert np.array_equal(same['samples'], np.zeros(50)) and same['value'] == 0.0 and same['fraction_a_better'] == 0.0
    assert same['low'] == same['high'] == 0.0
    with pytest.raises(ValueError):
        experiments.paired_bootstrap(a, b[:5])


def test_one_image_has_no_spread():
    cms = _per_image(1, 9)
    got = experiments.bootstrap_measure(cms, num_resamples=20)
    assert got['low'] == got['value'] == got['high'] and np.all(got['samples'] == got['value'])
    with pytest.raises(ValueError):
        experiments.bootstrap_measure(np.zeros((0, C, C)))


def test_measures_helper_is_the_formulas_of_score_with_an_empty_class():
    cm = _per_image(1, 4)[0]
    m = base_model.score_measures(cm)
    diag, rows, cols = np.diag(cm), cm.sum(1), cm.sum(0)
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = diag / (rows + cols - diag)
        precision, recall = diag / cols, diag / rows
        f1 = 2 * precision * recall / (precision + recall)
    assert np.isnan(iou[3]) and np.isnan(m['IoU'][3]) and np.isnan(m['F1'][3])
    for name, ref in (('IoU', iou), ('precision', precision), ('recall', recall), ('F1', f1)):
        assert np.array_equal(m[name], ref, equal_nan=True), name
    assert m['mean_IoU'] == np.nanmean(iou[1:]) and m['mean_F1'] == np.nanmean(f1)
    assert m['total_accuracy'] == diag[1:].sum() / cm[1:].sum()
    assert np.array_equal(m['confusion_matrix'], cm)
    # score() and score_groups() both go through it
    src = open(os.path.join(ROOT, 'modular_semantic_segmentation_amd', 'base_model.py')).read()
    body = lambda name: re.search(r'    def %s\(.*?(?=\n    def |\Z)' % name, src, re.S).group(0)      # noqa: E731
    assert 'score_measures(' in body('score') and 'grouped_results(' in body('score_groups')
    assert 'score_measures(' in re.search(r'\ndef grouped_results\(.*?(?=\n\ndef )', src, re.S).group(0)


class _StubNet(object):
    """score_groups of a network whose every image scores its own matrix"""

    def __init__(self, cms):
        self.cms = cms

    def score_groups(self, data, groups, max_iterations=None):
        keys, ids = base_model.dense_group_ids(groups)
        sums = np.zeros((len(keys),) + self.cms.shape[1:])
        np.add.at(sums, ids, self.cms)
        return base_model.grouped_results(keys, ids, len(ids), sums)


def test_evaluate_on_all_sequences_prints_one_line_per_sequence(capsys):
    cms = _per_image(5, 6, empty_class=False)
    sequences = ['SEQS-04-SUMMER', 'SEQS-02-FALL', 'SEQS-04-SUMMER', 'SEQS-02-FALL', 'SEQS-05-DAWN']
    out = experiments.evaluate_on_all_sequences(_StubNet(cms), {'labels': np.zeros((5, 2, 2))}, sequences)
    lines = capsys.readouterr().out.splitlines()
    assert list(out) == ['SEQS-04-SUMMER', 'SEQS-02-FALL', 'SEQS-05-DAWN']
    assert lines == ['Evaluated network on {}: {:.2f} IoU'.format(s, out[s]['mean_IoU']) for s in out]
    assert out['SEQS-02-FALL']['mean_IoU'] == base_model.score_measures(cms[1] + cms[3])['mean_IoU']
    results = experiments.evaluate_groups(_StubNet(cms), None, sequences, labelinfo={1: {'name': 'road'}})
    printed = capsys.readouterr().out.splitlines()
    assert len(printed) == 6 and printed[0].startswith('SEQS-04-SUMMER: total accuracy') and 'road' in printed[1]
    assert np.array_equal(results['SEQS-05-DAWN'][1], cms[4])
    assert experiments.evaluate_groups(_StubNet(cms), None, sequences, print_results=False) and capsys.readouterr().out == ''


def test_keys_become_dense_ids_in_first_seen_order():
    keys, ids = base_model.dense_group_ids(['b', ('a', 1), 'b', 7, ('a', 1)])
    assert keys == ['b', ('a', 1), 7] and ids.tolist() == [0, 1, 0, 2, 1] and ids.dtype == np.int64
    data, keys, ids = base_model.image_groups({'labels': np.zeros((5, 2, 2))}, 'image', None, 2)
    assert keys == [0, 1, 2, 3, 4] and ids.tolist() == keys
    assert base_model.image_groups({'labels': np.zeros((5, 2, 2))}, 'image', 2, 2)[1] == [0, 1, 2, 3]
    samples = ({'labels': np.zeros((2, 2))} for _ in range(3))                # an iterable without a length is read once
    data, keys, _ = base_model.image_groups(samples, 'image', None, 2)
    assert keys == [0, 1, 2] and len(data) == 3
    with pytest.raises(ValueError):
        base_model.image_groups({'labels': np.zeros((5, 2, 2))}, 'images', None, 2)
    with pytest.raises(ValueError, match='names 3 images'):                  # a pass over every image saw another number
        base_model.grouped_results(['a'], np.zeros(3, np.int64), 2, np.zeros((1, C, C)))
    assert list(base_model.grouped_results(['a', 'b'], np.array([0, 1, 1]), 1, np.zeros((2, C, C)), complete=False)) == ['a']


def test_new_entry_points_follow_the_abi_conventions():
    """What tests/test_host_logic.py holds every declaration to, for the two grouped entry points: derived ctypes signatures
    of the declared parameters, one definition, in csrc/grouped_score.hip, which reaches the header through xv_common.h."""
    from ctypes import c_int, c_int64, c_void_p
    p = c_void_p
    assert _lib.SIGNATURES['xv_confusion_matrix_grouped'] == (c_int, [p, p, p, c_int, c_int64, c_int, c_int, p, p])
    assert _lib.SIGNATURES['xv_fused_head_joint_hist_grouped_fwd'] == (
        c_int, [p, p, p, p, c_int, c_int, c_int, c_int, p, p, c_int, p, c_int, p])
    csrc = os.path.join(ROOT, 'modular_semantic_segmentation_amd', 'csrc')
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith('.hip')}
    assert '#include "xv_common.h"' in sources['grouped_score.hip']
    for name in ('xv_confusion_matrix_grouped', 'xv_fused_head_joint_hist_grouped_fwd'):
        where = [f for f, text in sources.items() if re.search(r'extern "C"\s+int\s+%s\s*\(' % name, text)]
        assert where == ['grouped_score.hip'], (name, where)
    mk = open(os.path.join(csrc, 'Makefile')).read()
    assert 'grouped_score.hip' in re.search(r'^SRCS := (.*)$', mk, re.M).group(1).split()
    assert 'xv_heads.h' in re.search(r'^HDRS := (.*)$', mk, re.M).group(1).split()     # hashed into xv_source_hash()
    from modular_semantic_segmentation_amd import ops
    assert callable(ops.confusion_matrix_grouped) and callable(ops.fused_head_joint_hist_grouped)


# ---- several ranks: one key table for all of them ---------------------------------------------------------------------------

class _HostNet(object):
    """BaseModel.score_groups over a counting pass on the host (numpy instead of the kernels): what is under test is the key
    table the ranks agree on and the reduction over it."""
    score_groups = base_model.BaseModel.score_groups

    def __init__(self, reduce):
        import torch
        self.config = {'batchsize': 2, 'num_classes': C, 'reduce_score_over_ranks': reduce}
        self.device = torch.device('cpu')

    def _count_groups(self, data, ids, num_groups, max_iterations, scored):
        import torch
        n = len(data['labels']) if max_iterations is None else min(len(data['labels']), 2 * max_iterations)
        cm = np.zeros((num_groups, C, C), np.int64)
        for i in range(n):
            ok = data['labels'][i] >= 0
            np.add.at(cm[ids[i]], (data['labels'][i][ok], data['pred'][i][ok]), 1)
        scored[0] = n
        t = torch.from_numpy(cm)
        base_model.reduce_over_ranks(self, t)
        return t.numpy()


RANK_KEYS = ['a', 'b', 'c', 'a', 'b', ('d', 1), 'c']       # three shards (3, 2, 2 images) see a b c | a b | d c


def _rank_dataset():
    rng = np.random.default_rng(8)
    n = len(RANK_KEYS)
    return {'labels': rng.integers(-1, C, (n, 6, 7)).astype(np.int32), 'pred': rng.integers(0, C, (n, 6, 7)).astype(np.int64)}


def _rank_worker(rank, size, port, out):
    import pickle
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=size)
    from modular_semantic_segmentation_amd import parallel
    full = _rank_dataset()
    b, e = parallel.shard_range(len(RANK_KEYS))
    data, keys = parallel.shard_data(full), RANK_KEYS[b:e]
    net = _HostNet(reduce=True)
    res = {'keys': net.score_groups(data, keys), 'image': net.score_groups(data, 'image'),
           'image_1': net.score_groups(data, 'image', max_iterations=1),
           'table': parallel.agree_group_keys(base_model.dense_group_ids(keys)[0]), 'range': parallel.agree_image_range(e - b)}
    with open(out % rank, 'wb') as f:
        pickle.dump({k: ({kk: vv[1] for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in res.items()}, f)
    dist.destroy_process_group()


def test_ranks_agree_on_one_key_table_and_every_rank_returns_every_key(tmp_path):
    import pickle
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'rank%d.pkl')
    mp.spawn(_rank_worker, args=(3, port, out), nprocs=3, join=True)
    got = [pickle.load(open(out % r, 'rb')) for r in range(3)]
    full = _rank_dataset()
    single = _HostNet(reduce=False)
    ref_keys = {k: v[1] for k, v in single.score_groups(full, RANK_KEYS).items()}
    ref_image = {k: v[1] for k, v in single.score_groups(full, 'image').items()}
    assert [g['range'] for g in got] == [(0, 7), (3, 7), (5, 7)]
    for g in got:
        assert g['table'] == ['a', 'b', 'c', ('d', 1)]                       # rank order; rank 2 alone would say d, c
        assert list(g['keys']) == ['a', 'b', 'c', ('d', 1)] and list(g['image']) == list(range(7))
        for key, cm in ref_keys.items():
            assert np.array_equal(g['keys'][key], cm), key
        for key, cm in ref_image.items():
            assert np.array_equal(g['image'][key], cm), key
        # one batch of two images per rank: global indices 0 1 | 2 3 | 4 5 of the scored images, the full set's images 0 1 3 4 5 6
        assert list(g['image_1']) == list(range(6))
        for key, src in zip(range(6), (0, 1, 3, 4, 5, 6)):
            assert np.array_equal(g['image_1'][key], ref_image[src]), key
    # one process: nothing is gathered
    from modular_semantic_segmentation_amd import parallel
    assert parallel.agree_group_keys(['x', 'y']) == ['x', 'y'] and parallel.agree_image_range(4) == (0, 4)
