"""FusionModel base + test_pipeline (reference: xview/models/basic_fusion_model.py)."""
from copy import deepcopy

import numpy as np
import torch

from .base_model import (BaseModel, grouped_batches, grouped_results, groups_seen, image_groups,  # noqa: F401
                         iterate_batches, reduce_over_ranks, score_measures)
from .fcn import FcnEngine, init_variables


def test_pipeline(engine, inputs, want=('prob', 'classification'), st=None):
    """Expert forward + softmax + argmax (basic_fusion_model.py:9-23) on an FcnEngine:
    returns {'prob': f32 [N,H,W,C], 'classification': i64 [N,H,W]} (only what `want` names).  st: an encoder state to
    finish (the shared launches of two experts, run_trunks) instead of `inputs`."""
    want = tuple('label' if w == 'classification' else w for w in want)
    return engine.forward(inputs, want=want, st=st) if st is not None else engine.forward(inputs, want=want)


def expert_factory(expert_model, conv_dtype='bf16'):
    """(engine class, initialiser) of an `expert_model` name, the choice test_pipeline makes
    (basic_fusion_model.py:13-20); conv_dtype='fp32': the plain-float32 FCN engine (fcn_exact, the parity mode)."""
    if expert_model == 'fcn':
        if conv_dtype == 'fp32':
            from .fcn_exact import FcnEngineF32
            return FcnEngineF32, init_variables
        return FcnEngine, init_variables
    if expert_model == 'adapnet':
        from .adapnet import AdapnetEngine, init_variables as init_adapnet
        return AdapnetEngine, init_adapnet
    raise UserWarning('ERROR: Expert Model %s not found' % expert_model)


def engine_options(config):
    """Extra constructor arguments of the expert engines named by the model config (conv_dtype: the fp8 conv path of
    the FCN expert, fp8_deep: e4m3 operands from conv1_2 on -- see fcn.fp8_plan; streamk: its split tail rounds, a batch-1
    latency option -- see FcnEngine; the AdapNet engine has none)."""
    opts = {}
    if config.get('expert_model', 'fcn') == 'fcn':
        if config.get('conv_dtype', 'bf16') != 'bf16':
            opts['conv_dtype'] = config['conv_dtype']
        if config.get('streamk', False):
            opts['streamk'] = True
        if config.get('fp8_deep', False):
            opts['fp8_deep'] = True
        if config.get('fp8_start'):
            opts['fp8_start'] = config['fp8_start']     # a layer name, or {prefix: layer name} per expert
    return opts


def fp8_guard_bound(config):
    """Label-agreement bound of the accuracy-guarded fp8 plan (FcnEngine.calibrate_guarded), or None where the plan is given:
    model config `fp8_agreement` (default fcn.FP8_GUARD_AGREEMENT = 0.995; 0 / None: off); an explicit `fp8_start` or
    `fp8_deep` is a plan of the caller's and is not second-guessed."""
    from .fcn import FP8_GUARD_AGREEMENT
    if config.get('fp8_start') or config.get('fp8_deep'):
        return None
    bound = config.get('fp8_agreement', FP8_GUARD_AGREEMENT)
    return float(bound) if bound else None


def calibrate_experts(model, data):
    """conv_dtype='fp8': fix every expert's activation scales from the first batch of `data` -- and, unless the config names
    a plan, choose every expert's e4m3 plan by its label agreement with the bf16 graph on that batch (fp8_guard_bound)."""
    from .base_model import iterate_batches
    batch = next(iterate_batches(data, model.config['batchsize']))
    model._graph = None
    bound = fp8_guard_bound(model.config)
    out = {}
    for m in model.modalities:
        x = model._to_device(batch[m], torch.float32)
        eng = model.experts[m]
        out[m] = eng.calibrate_guarded(x, bound) if bound is not None and hasattr(eng, 'calibrate_guarded') else eng.calibrate(x)
    return out


def fp8_plan_report(model):
    """{modality: the engine's calibrate_guarded report or its fixed plan} of an fp8 model (bench records, logs)."""
    rep = {}
    for m in model.modalities:
        eng = model.experts[m]
        rep[m] = eng.fp8_guard if getattr(eng, 'fp8_guard', None) else {
            'chosen': 'bf16' if getattr(eng, 'fp8_off', False) else (getattr(eng, 'fp8_start', None) or ('conv1_2' if getattr(eng, 'fp8_deep', False) else 'conv2_2')),
            'bound': None}
    return rep


def fills_the_chip(model, inputs, rounds=1):
    """Does ONE expert's conv4 map give at least `rounds` rounds of workgroups (16x32-pixel x 64-channel tiles against the CU
    count)?"""
    shapes = {tuple(v.shape[:3]) for v in inputs.values()}
    if len(shapes) != 1:
        return False
    n, h, w = next(iter(shapes))
    tiles = n * ((h // 8 + 15) // 16) * ((w // 8 + 31) // 32) * 8
    return tiles >= rounds * torch.cuda.get_device_properties(model.device).multi_processor_count


def expert_streams(model, inputs):
    """Run the experts side by side on two HIP streams?  model.concurrent_experts: True / False force it; None (default): two
    streams while the launches of one expert leave CUs idle or end in half-empty rounds (2 / 4 / 8 images of 768x384: 2 958 /
    3 406 / 3 552 images/s against 2 176 / 3 051 / 3 461 on one stream), ONE stream from three rounds of conv4 workgroups
    per expert on (12 images: 3 685 against 3 568; 16 images: 3 799-3 829 against 3 636-3 698 on one box, 3 735 against
    3 574-3 617 on another): there every launch fills the chip for several rounds, and two queues only make the persistent
    grids of two kernels share CUs.  Same kernels, same bits either way."""
    conc = getattr(model, 'concurrent_experts', None)
    if conc is None:
        conc = not fills_the_chip(model, inputs, rounds=3)
    return bool(conc)


def paired_from(model, inputs):
    """Index of the first encoder layer the two experts run as ONE launch each (fcn.encoder_layers_pair), or None: two FCN
    experts on the bf16 path without dropout sites or the stream-K option -- and a batch whose conv4 maps give one expert
    at least one round of workgroups (16x32-pixel x 64-channel tiles against the CU count).  Below that the launches are
    latency: both experts' kernels fit the chip side by side on their two streams, and the joins of a paired section only
    cost (one image: 0.46 -> 0.49 ms per step with it)."""
    from .fcn import group_from_index
    gi = group_from_index()
    if gi is None or len(model.modalities) != 2 or not model.config.get('paired_launches', True):
        return None
    if not all(type(e) is FcnEngine and e.pairable() for e in model.experts.values()):
        return None
    # (modalities of different sizes cannot share a launch: both stay on their own streams)
    if not fills_the_chip(model, inputs):
        return None
    return gi


def run_trunks(model, inputs, finish, pair=True):
    """Both experts up to finish(modality, state-or-None) -> result: each on its own HIP stream (the experts are independent
    until the fusion kernel); from paired_from() on the layers both experts share are ONE launch each on the current stream
    -- whole rounds of workgroups where each expert alone leaves its last round half empty -- and the streams fork again for
    the heads.  The current stream waits for all of them before returning.  pair=False: no paired section (finish runs the
    whole trunk of each expert on its own)."""
    from .fcn import encoder_layers_pair
    mods = model.modalities
    conc = expert_streams(model, inputs)
    main = torch.cuda.current_stream(model.device)
    if conc and not hasattr(model, '_expert_streams'):
        model._expert_streams = {m: torch.cuda.Stream(device=model.device) for m in mods}

    def each(fn):
        out = {}
        for m in mods:
            if conc:
                side = model._expert_streams[m]
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    out[m] = fn(m)
            else:
                out[m] = fn(m)
        if conc:
            for m in mods:
                main.wait_stream(model._expert_streams[m])
        return out

    gi = paired_from(model, inputs) if pair else None
    if gi is None:
        return each(lambda m: finish(m, None))
    st = each(lambda m: model.experts[m].encoder_begin(inputs[m], stop=gi))
    a, b = mods
    encoder_layers_pair(model.experts[a], st[a], model.experts[b], st[b])
    return each(lambda m: finish(m, st[m]))


def run_experts(model, batch, wants):
    """Forward every modality's expert (run_trunks), each to its test_pipeline outputs."""
    inputs = {m: model._to_device(batch[m], torch.float32) for m in model.modalities}
    main = torch.cuda.current_stream(model.device)

    def finish(m, st):
        out = test_pipeline(model.experts[m], inputs[m], want=wants, st=st)
        for v in out.values():
            if isinstance(v, torch.Tensor):
                v.record_stream(main)
        return out
    return run_trunks(model, inputs, finish)


def fused_head_applicable(model):
    """The fused two-expert head (ops.fused_head) serves the default prediction of a fusion model with two FCN experts
    whose decoder heads are in the commuted form; config fused_head=False keeps the per-expert outputs
    (`expert_outputs`, `probs`) materialised as the unfused path does."""
    if not model.config.get('fused_head', True) or len(model.modalities) != 2:
        return False
    return all(isinstance(e, FcnEngine) and e.commuted_head() for e in model.experts.values())


MULTI_HEAD_EXPERTS = (3, 4)         # xv_fused_head_multi_fwd takes two to four; two experts keep the two-expert heads


def multi_head_applicable(model):
    """The fused head for three or four experts (ops.fused_head_multi) serves the default prediction of a fusion model with
    that many FCN experts whose decoder heads are in the commuted form; config fused_head=False keeps the per-expert outputs
    materialised.  Two experts are fused_head_applicable's; five or more fuse materialised outputs."""
    if not model.config.get('fused_head', True) or len(model.modalities) not in MULTI_HEAD_EXPERTS:
        return False
    return all(isinstance(e, FcnEngine) and e.commuted_head() for e in model.experts.values())


def tuple_head_applicable(model):
    """The label-tuple heads (ops.fused_head_multi_lut, its counting form and ops.fused_head_multi_tuple_hist) serve a fusion
    that decides by the tuple of its experts' labels (IbccFusion) with two to four FCN experts whose decoder heads are in the
    commuted form, while the C^E counters of the pair fit one workgroup's LDS (ops.tuple_capacity); config fused_head=False
    keeps the experts' label maps materialised."""
    from . import ops
    if not model.config.get('fused_head', True) or not 2 <= len(model.modalities) <= 4:
        return False
    if not all(isinstance(e, FcnEngine) and e.commuted_head() for e in model.experts.values()):
        return False
    return ops.tuple_capacity(model.config['num_classes'], len(model.modalities))


def run_lowres_scores_multi(model, batch):
    """Every trunk on its own stream (run_trunks without a paired section) up to its low-resolution class scores:
    (scores, biases, n, hi, wi) with one entry per modality, in the model's order -- what ops.fused_head_multi takes."""
    inputs = {m: model._to_device(batch[m], torch.float32) for m in model.modalities}
    res = run_trunks(model, inputs, lambda m, st: model.experts[m].lowres_scores(inputs[m], st=st), pair=False)
    n, hi, wi = res[model.modalities[0]][1]
    if any(res[m][1] != (n, hi, wi) for m in model.modalities):
        raise ValueError('the experts disagree on the size of their low-resolution scores: %s' % {m: res[m][1] for m in model.modalities})
    return ([res[m][0] for m in model.modalities], [model.experts[m].b['score'] for m in model.modalities], n, hi, wi)


def _head_arguments(model, res):
    """(Sa, Sb, bias_a, bias_b, n, hi, wi), what the two-expert heads take, from {modality: (scores, (n, hi, wi))}."""
    a, b = model.modalities
    n, hi, wi = res[a][1]
    return res[a][0], res[b][0], model.experts[a].b['score'], model.experts[b].b['score'], n, hi, wi


def run_lowres_scores(model, batch):
    """Both trunks (run_trunks) up to their low-resolution class scores: (Sa, Sb, bias_a, bias_b, n, hi, wi), what the fused
    heads take."""
    inputs = {m: model._to_device(batch[m], torch.float32) for m in model.modalities}
    return _head_arguments(model, run_trunks(model, inputs, lambda m, st: model.experts[m].lowres_scores(inputs[m], st=st)))


# ---- MC dropout: what VarianceFusion, UncertaintyMix and BayesianFCN share ---------------------------------------------------

def mc_dropout_setup(name, config, strict=False, fusion=True, engines=()):
    """Validate the MC-dropout keys of `config` for the model `name` and return (dropout_rate, num_samples, seed of the masks:
    dropout_seed, else seed, else 0).  A model calls it on its raw config before anything is built -- every refusal that needs
    no engine comes before a device is touched -- and again with the built `engines`, which must run the commuted decoder
    head and are given the config's mc_chunk_images (default 64).  strict: a model that divides by the samples' variance
    needs some (a rate in (0, 1), two samples) where the others take rate 0 and one sample; fusion: the model samples
    experts, which must be FCNs."""
    for key in ('dropout_rate', 'num_samples'):
        if key not in config:
            raise UserWarning('ERROR: %s needs %s in its config' % (name, key))
    if fusion and config.get('expert_model', 'fcn') != 'fcn':
        raise UserWarning('ERROR: %s samples FCN experts only (expert_model=%r)' % (name, config['expert_model']))
    rate, T = float(config['dropout_rate']), int(config['num_samples'])
    if strict:
        if not 0.0 < rate < 1.0:
            raise ValueError('dropout_rate must lie in (0, 1): without dropout there is no variance to weigh the experts by')
        if T < 2:
            raise ValueError('num_samples must be at least 2: one sample has no variance')
    elif not 0.0 <= rate < 1.0 or T < 1:
        raise ValueError('dropout_rate must lie in [0, 1) and num_samples be at least 1')
    for e in engines:
        if not e.commuted_head():
            raise NotImplementedError('%s needs experts with the commuted decoder head (bilinear x8 deconv)' % name)
        e.mc_chunk_images = int(config.get('mc_chunk_images', 64))
    seed = config.get('dropout_seed', config.get('seed'))
    return rate, T, int(seed) if seed is not None else 0


def run_mc_lowres_scores(model, batch, sampler):
    """run_lowres_scores of an MC-dropout fusion: the engine method named `sampler` ('mc_lowres_scores', 'mc_input_scores')
    gives each expert's plain pass and its num_samples dropped passes as one slot-major score tensor, every expert under
    masks of its own (seed + its index).  Every call draws new masks: such a model never captures its step (_graph_capturable)."""
    inputs = {m: model._to_device(batch[m], torch.float32) for m in model.modalities}
    rate, T = float(model.config['dropout_rate']), int(model.config['num_samples'])
    seeds = {m: model._dropout_seed + i for i, m in enumerate(model.modalities)}
    # pair=False: the samplers run their own trunks -- a paired section would skip the replication at the dropout site
    return _head_arguments(model, run_trunks(
        model, inputs, lambda m, st: getattr(model.experts[m], sampler)(inputs[m], T, rate, seeds[m]), pair=False))


def per_expert_output(model, t, keep=None):
    """An optional output of a two-expert head, [E, N, ...], as predict returns it: [N, E, ...]; keep: the attribute that
    holds {modality: its slice} afterwards (`probs`, `variances`)."""
    if keep is not None:
        setattr(model, keep, {m: t[i] for i, m in enumerate(model.modalities)})
    return t.transpose(0, 1).contiguous()


# ---- small change shared by the *_mix modules --------------------------------------------------------------------------------

def device_tables(device, *tables):
    """The numpy tables of a fusion (bayes_tables, dirichlet_tables, ...) as device tensors, in order."""
    return tuple(torch.from_numpy(t).to(device) for t in tables)


def output_key(output_attr):
    """The one name of an optional output: 'score' is 'fused_score', 'prob' is 'probs'; anything else is itself."""
    return {'score': 'fused_score', 'prob': 'probs'}.get(output_attr, output_attr)


# ---- grid search over the fusion parameters in ONE pass of the experts (experiments/different_evaluation_parameters.py) ------
# The reference builds and evaluates one model per grid point.  The parameters of the fusion itself (class prior, sigma, the
# regularisation of the Dirichlet fit) never reach the experts, so a fusion model scores all of them on one pass: the experts
# run once per batch and only the fusion and the counting are repeated -- inside one kernel where the fused head serves the
# model (score_grid_fused; score_grid_fused_multi for three or four experts), through the fusion kernels on the experts'
# materialised outputs otherwise (score_grid_generic).
# Both count the same integers.  The pass runs eagerly (no hipGraph capture: it is not the step predict() replays).

def parameter_combinations(search_parameters, net_config):
    """Every combination of the searched values as a full config: copies of `net_config` with the searched keys replaced.
    The FIRST key of `search_parameters` varies slowest, the last one fastest."""
    configs = [net_config]
    for key, values in search_parameters.items():
        configs = [dict(deepcopy(config), **{key: value}) for config in configs for value in values]
    return configs


def grid_point_configs(model, search_parameters, searchable):
    """parameter_combinations over the model's own config, after refusing what one pass cannot vary: any key outside
    `searchable` changes the experts or the data flow and needs a model per grid point (experiments.grid_search)."""
    for key in search_parameters:
        if key not in searchable:
            raise ValueError('score_grid of %s cannot search %r in one pass (searchable: %s); build one model per grid point '
                             'with experiments.grid_search' % (type(model).__name__, key, ', '.join(searchable)))
    return parameter_combinations(search_parameters, model.config)


def _labelled_batches(model, data, max_iterations):
    for batch in model._device_batches(iterate_batches(data, model.config['batchsize'], max_iterations), labels=True):
        yield batch, model._to_device(batch['labels'], torch.int32)


def score_grid_fused(model, data, counts, count_batch, max_iterations=None):
    """The fused route: per batch both trunks once (run_lowres_scores), then count_batch(Sa, Sb, bias_a, bias_b, n, hi, wi,
    labels, counts) accumulates into the device tensor `counts`."""
    for batch, labels in _labelled_batches(model, data, max_iterations):
        count_batch(*run_lowres_scores(model, batch), labels, counts)
    return counts


def score_grid_fused_multi(model, data, mode, num_points, max_iterations=None, **tables):
    """The fused route of three or four experts (multi_head_applicable): per batch every trunk once up to its low-resolution
    scores (run_lowres_scores_multi), then ONE ops.fused_head_multi_count launch fuses every pixel under all `num_points`
    parameter sets (`tables`: tab, lognorm, logprior as that op takes them for `mode`) and counts it.  Returns the int64
    [G, C, C] counts."""
    from . import ops
    C = model.config['num_classes']
    counts = torch.zeros((num_points, C, C), dtype=torch.int64, device=model.device)
    for batch, labels in _labelled_batches(model, data, max_iterations):
        ops.fused_head_multi_count(*run_lowres_scores_multi(model, batch), C, mode, labels, cm=counts, **tables)
    return counts


def score_grid_generic(model, data, num_points, wants, fuse_point, max_iterations=None):
    """The generic route (any experts, any number of them): per batch every expert once (run_experts), then per grid point g
    fuse_point(expert outputs, g) -> fused labels, counted by ops.confusion_matrix.  Returns the int64 [G, C, C] counts."""
    from . import ops
    C = model.config['num_classes']
    counts = torch.zeros((num_points, C, C), dtype=torch.int64, device=model.device)
    for batch, labels in _labelled_batches(model, data, max_iterations):
        outs = run_experts(model, batch, wants)
        for g in range(num_points):
            ops.confusion_matrix(labels, fuse_point(outs, g).contiguous(), counts[g])
    return counts


def measure_experts(model, data, confusion=False):
    """One pass of the experts over the labelled batches of `data` (dirichlet_mix.py:175-205): per modality the Dirichlet
    sufficient statistics S[c,k] = sum_{label=c} log(1e-10 + p[k]) (float64 [C,C]), the class counts (int64 [C]) and, with
    confusion=True, every expert's confusion matrix (int64 [C,C], rows = ground truth).  Returns (S, counts, matrices or None)
    on the device, this rank's share: the caller sums over ranks."""
    from . import ops
    C, mods = model.config['num_classes'], model.modalities
    S = {m: torch.zeros((C, C), dtype=torch.float64, device=model.device) for m in mods}
    cms = {m: torch.zeros((C, C), dtype=torch.int64, device=model.device) for m in mods} if confusion else None
    counts = torch.zeros(C, dtype=torch.int64, device=model.device)
    scratch = torch.zeros(C, dtype=torch.int64, device=model.device)     # every expert sees the same labels: count them once
    wants = ('classification', 'prob') if confusion else ('prob',)
    for batch, labels in _labelled_batches(model, data, None):
        outs = run_experts(model, batch, wants)
        for i, m in enumerate(mods):
            if confusion:
                ops.confusion_matrix(labels, outs[m]['classification'].contiguous(), cms[m])
            ops.dirichlet_suffstats(outs[m]['prob'], labels, S[m], counts if i == 0 else scratch)
    return S, counts, cms


def grid_results(configs, confusion_matrices):
    """[(point config, measures, confusion matrix float64 [C, C])] per grid point, each pair as score() returns it."""
    out = []
    for config, cm in zip(configs, confusion_matrices):
        cm = np.asarray(cm).astype(np.float64)
        out.append((config, score_measures(cm), cm))
    return out


# ---- expert agreement: who is right and whom the fusion follows (csrc/agreement.hip) ----------------------------------------
# A confusion matrix is a marginal of one method.  The agreement table keeps, per ground-truth class, what matters of the JOINT
# of the experts' labels and the fused one: table[label][mask][unanimous][outcome], int64 [C, 2^E, 2, 3], with bit e of mask set
# iff expert e is right, unanimous = 1 iff all experts give one label, outcome 0 = the fused label is right, 1 = wrong but some
# expert's label, 2 = wrong and no expert's label.

AGREEMENT_MAX_EXPERTS = 4


def _agreement_shares(t, names):
    """The measures of agreement_measures for K tables at once: t float64 [K, 2^E, 2, 3] -> {key: float64 [K]}; a table
    without pixels gives NaN."""
    E = t.shape[1].bit_length() - 1
    masks = np.arange(t.shape[1])
    pixels = t.sum((1, 2, 3))
    split = t[:, :, 0].sum((1, 2))                                      # pixels on which the experts do not all agree
    with np.errstate(divide='ignore', invalid='ignore'):
        out = {'pixels': pixels,
               'fused_accuracy': t[..., 0].sum((1, 2)) / pixels,
               'expert_accuracy': {names[e]: t[:, (masks >> e) & 1 == 1].sum((1, 2, 3)) / pixels for e in range(E)},
               'oracle_accuracy': t[:, 1:].sum((1, 2, 3)) / pixels,
               'unanimous': t[:, :, 1].sum((1, 2)) / pixels,
               'fused_accuracy_on_disagreement': t[:, :, 0, 0].sum(1) / split,
               'rescued': t[:, 0, :, 0].sum(1) / pixels,
               'lost': t[:, 1:, :, 1:].sum((1, 2, 3)) / pixels,
               'own_way_errors': t[..., 2].sum((1, 2)) / pixels}
        out['best_expert_accuracy'] = np.max(np.stack(list(out['expert_accuracy'].values())), 0)
        if E == 2:
            # the experts differ; expert e alone is right (mask 1 << e): outcome 0 follows e, outcome 1 the other one.  Both
            # wrong (mask 0): outcome 1 follows one of them, and the table does not say which
            out['follows'] = {names[e]: (t[:, 1 << e, 0, 0] + t[:, 2 >> e, 0, 1]) / split for e in range(2)}
            out['follows_undecided'] = t[:, 0, 0, 1] / split
    return out


def agreement_measures(table, modalities=None):
    """Measures of one expert-agreement table (int [C, 2^E, 2, 3], as score_agreement returns it), pure numpy:
      pixels                          the pixels counted (0 <= label < C)
      fused_accuracy                  outcome 0
      expert_accuracy                 {expert: share of the pixels it labels right}, keyed by `modalities` (else 0 .. E-1)
      best_expert_accuracy            the largest of them
      oracle_accuracy                 some expert is right (mask != 0): what a fusion that always picks a right expert reaches
      unanimous                       all experts give the same label
      fused_accuracy_on_disagreement  outcome 0 among the pixels with unanimous = 0 (NaN when there are none)
      rescued                         no expert is right, the fused label is (mask = 0, outcome 0)
      lost                            some expert is right, the fused label is not (mask != 0, outcome != 0)
      own_way_errors                  the fused label is wrong and no expert's (outcome 2)
    all but `pixels` and the disagreement accuracy as shares of the pixels.  Two experts only: `follows`, {expert: share of the
    non-unanimous pixels on which the fused label equals that expert's}, as far as the table decides it -- where both experts
    are wrong, differ, and the fusion takes one of the two labels, the table does not say whose: that share is
    `follows_undecided` and is in neither entry of `follows`.  For three or more experts the table says even less about whom a
    wrong fused label follows, and both keys are left out.  `per_class`: the same keys per ground-truth class (arrays [C]; a
    class without pixels gives NaN, as the measures of score() do)."""
    t = np.asarray(table).astype(np.float64)
    if t.ndim != 4 or t.shape[2:] != (2, 3) or t.shape[1] not in (4, 8, 16):
        raise ValueError('agreement table of shape %s, expected [C, 2^E, 2, 3] with E in 2..4' % (t.shape,))
    E = t.shape[1].bit_length() - 1
    names = list(modalities) if modalities is not None else list(range(E))
    if len(names) != E:
        raise ValueError('%d modalities for a table of %d experts' % (len(names), E))

    def first(v):
        return {k: first(x) for k, x in v.items()} if isinstance(v, dict) else float(v[0])
    measures = first(_agreement_shares(t.sum(0, keepdims=True), names))
    measures['per_class'] = _agreement_shares(t, names)
    return measures


class FusionModel(BaseModel):
    """Mixture of per-modality experts, which this class builds and owns; subclasses implement `_fusion(expert_outputs)` and
    may name a fused head.  config: prefixes {modality: prefix} or modalities (a list: every expert's prefix is its modality,
    dirichlet_mix.py:98), num_units, num_channels {modality: C_in}, expert_model."""

    expert_wants = ('classification',)
    has_fused_score = False         # _fusion(..., output_attr='fused_score') returns the fused class scores
    agreement_refusal = None        # why score_agreement does not serve the model (the MC-dropout fusions), or None

    def __init__(self, name=None, output_dir=None, **config):
        self.modalities = list(config['prefixes'] if 'prefixes' in config else config['modalities'])
        BaseModel.__init__(self, name=name, output_dir=output_dir, custom_training=True, **config)

    def _fusion(self, expert_outputs, output_attr=None):
        raise NotImplementedError

    def _fused_head(self):
        """The model's head for both experts' low-resolution scores -- head(Sa, Sb, bias_a, bias_b, n, hi, wi) -> fused
        labels in ONE kernel, per-expert softmax / argmax included -- or None: it fuses materialised expert outputs only."""
        return None

    def _multi_head(self):
        """The model's head for three or four experts' low-resolution scores -- head(scores, biases, n, hi, wi) -> fused
        labels in ONE kernel (ops.fused_head_multi) -- or None: it fuses materialised expert outputs only."""
        return None

    def _build_experts(self):
        """Hook: fills self.experts {modality: engine} and self.variables (a test without a GPU overrides it)."""
        engine_cls, init = expert_factory(self.config['expert_model'], self.config.get('conv_dtype', 'bf16'))
        self.experts = {}
        for m in self.modalities:
            prefix = self.config['prefixes'][m] if 'prefixes' in self.config else m
            cin = self._modality_channels(m)
            # experts run with trainable=False, batchnorm=False (basic_fusion_model.py:17-18)
            self.variables.update(init(prefix, cin, self.config['num_units'], self.config['num_classes'],
                                       seed=self.config.get('seed')))
            self.experts[m] = engine_cls(prefix, cin, self.config['num_units'], self.config['num_classes'],
                                         self.variables, device=self.device, **engine_options(self.config))

    def _build_graph(self):
        # ONCE per model object: a model that refits its tables calls _initialize_graph() again (DirichletFusion.fit), and a
        # second build would re-draw the variables and discard imported weights
        if not hasattr(self, 'experts'):
            self._build_experts()
        self.prediction = 'fused_label'

    def _modality_channels(self, m):
        if 'num_channels' in self.config:
            return int(self.config['num_channels'][m])
        return int(self.testdata_description[1][m][-1])

    def _variables_changed(self):
        BaseModel._variables_changed(self)
        for m in self.modalities:
            self.experts[m].load(self.variables)

    def calibrate(self, data):
        return calibrate_experts(self, data)

    def _predict_batch_impl(self, batch, output_attr=None):
        head = self._fused_head() if output_attr is None else None
        if head is not None and fused_head_applicable(self):
            # default prediction: nothing but the fused label map is wanted -> one head kernel after the trunks; the experts'
            # labels and probabilities never leave its registers
            self.expert_outputs = None
            return head(*run_lowres_scores(self, batch))
        head = self._multi_head() if output_attr is None else None
        if head is not None and multi_head_applicable(self):
            # the same for three or four experts: every trunk on its own stream, then one head kernel for all of them
            self.expert_outputs = None
            return head(*run_lowres_scores_multi(self, batch))
        key = output_key(output_attr)
        wants = self.expert_wants
        if key == 'probs' and 'prob' not in wants:
            wants = tuple(wants) + ('prob',)
        self.expert_outputs = run_experts(self, batch, wants)
        return self._fusion(self.expert_outputs, output_attr=key)

    # ---- expert agreement on one pass ---------------------------------------------------------------------------------------
    def _agreement_head(self):
        """(mode, tables) of ops.fused_head_multi_agreement for this model's fusion -- ('bayes' | 'dirichlet' | 'mean', {tab,
        lognorm, logprior as that op takes them}) -- or None: the model's agreement is counted from materialised maps only."""
        return None

    def _count_agreement(self, data, ids, num_groups, max_iterations, scored):
        """int64 [G, C, 2^E, 2, 3] on the host from ONE pass over `data`.  Where a fused head serves the model (two to four
        commuted FCN experts, fused_head not switched off) the trunks stop at their low-resolution scores and one
        ops.fused_head_multi_agreement launch per batch counts; otherwise the experts' label maps are materialised, fused by the
        model's _fusion and counted by ops.agreement_table.  ids None: one group, every image."""
        from . import ops
        C, E = self.config['num_classes'], len(self.modalities)
        table = torch.zeros((num_groups, C, 1 << E, 2, 3), dtype=torch.int64, device=self.device)
        head = self._agreement_head()
        fused_route = head is not None and (fused_head_applicable(self) or multi_head_applicable(self))
        wants = tuple(dict.fromkeys(tuple(self.expert_wants) + ('classification',)))
        if ids is None:
            batches = ((batch, labels, None) for batch, labels in _labelled_batches(self, data, max_iterations))
        else:
            batches = grouped_batches(self, data, ids, num_groups, max_iterations, scored)
        for batch, labels, batch_ids in batches:
            into = dict(table=table[0]) if batch_ids is None else dict(groups=batch_ids, num_groups=num_groups, table=table)
            if fused_route:
                ops.fused_head_multi_agreement(*run_lowres_scores_multi(self, batch), C, head[0], labels, **head[1], **into)
            else:
                outs = run_experts(self, batch, wants)
                fused = self._fusion(outs, output_attr=None)
                ops.agreement_table(labels, [outs[m]['classification'].contiguous() for m in self.modalities],
                                    fused.contiguous(), C, **into)
        reduce_over_ranks(self, table)
        return table.cpu().numpy()

    def score_agreement(self, data, groups=None, max_iterations=None):
        """(measures, table) over `data`: the expert-agreement table int64 [C, 2^E, 2, 3] (agreement_measures says what it
        holds; the experts in the order of self.modalities) from one pass, and its measures.  With `groups` -- one hashable key
        per image in data order, or 'image', as score_groups takes them, the key table agreed over the ranks the same way --
        {key: (measures, table)}, each pair what the call returns for the images of that key alone.  Summed over the ranks
        under reduce_score_over_ranks like the other counting scores.  Two to four experts; the MC-dropout fusions are not
        served (NotImplementedError)."""
        if self.agreement_refusal is not None:
            raise NotImplementedError('%s.score_agreement: %s' % (type(self).__name__, self.agreement_refusal))
        E = len(self.modalities)
        if not 2 <= E <= AGREEMENT_MAX_EXPERTS:
            raise NotImplementedError('score_agreement takes two to %d experts (a table of 2^E masks per class), this model '
                                      'has %d' % (AGREEMENT_MAX_EXPERTS, E))
        if groups is None:
            table = self._count_agreement(data, None, 1, max_iterations, [0])[0]
            return agreement_measures(table, self.modalities), table
        data, keys, ids = image_groups(data, groups, max_iterations, self.config['batchsize'],
                                       across_ranks=self.config.get('reduce_score_over_ranks', False))
        if not keys:
            return {}
        scored = [0]
        tables = self._count_agreement(data, ids, len(keys), max_iterations, scored)
        return grouped_results(keys, ids, scored[0], tables, complete=max_iterations is None,
                               result=lambda t: (agreement_measures(t, self.modalities), np.asarray(t)),
                               seen=groups_seen(self, ids, scored[0], len(keys)))

    # ---- calibration of the fused posterior on one pass (BaseModel.score_calibration, csrc/calibration.hip) ----------------
    def _calibration_refusal(self):
        return self.calibration_refusal if self.calibration_refusal is not None else self.agreement_refusal

    def _calibration_experts(self):
        return self.modalities

    def _calibration_values(self, expert_outputs):
        """(values float32 [N, H, W, C], kind) of the materialised route: the fused class scores in the log domain (kind 0) --
        the model's fusion with output_attr='fused_score' -- or, kind 1, the probabilities it decides by (AverageFusion)."""
        if not self.has_fused_score:
            raise NotImplementedError('%s.score_calibration: the fusion has no class scores' % type(self).__name__)
        return self._fusion(expert_outputs, output_attr='fused_score'), 0

    def _calibrate_batch(self, batch, labels, temps, bin_bits, into, expert_into):
        """Where a fused head serves the model (two to four commuted FCN experts, fused_head not switched off) the trunks stop
        at their low-resolution scores and ONE ops.fused_head_multi_calibration launch counts the fused table and, on request,
        every expert's; otherwise the experts' outputs are materialised, fused by the model's own kernel with its score output
        and counted by ops.calibration_table, every expert's table from its materialised class scores."""
        from . import ops
        C = self.config['num_classes']
        head = self._agreement_head()
        if head is not None and (fused_head_applicable(self) or multi_head_applicable(self)):
            ops.fused_head_multi_calibration(*run_lowres_scores_multi(self, batch), C, head[0], labels, temps, bin_bits,
                                             **head[1], **into, **(expert_into or {}))
            return
        wants = tuple(dict.fromkeys(tuple(self.expert_wants) + (('score',) if expert_into else ())))
        outs = run_experts(self, batch, wants)
        values, kind = self._calibration_values(outs)
        ops.calibration_table(values.contiguous(), labels, temps, bin_bits, kind=kind, **into)
        if expert_into:
            grouped = 'groups' in into
            for e, m in enumerate(self.modalities):
                # (a grouped expert table [G, E, T, NB, 3] has no dense slice per expert: counted apart, then added)
                part, part_nll = ops.calibration_table(
                    outs[m]['score'].contiguous(), labels, temps, bin_bits, kind=0,
                    **(dict(groups=into['groups'], num_groups=into['num_groups']) if grouped else
                       dict(table=expert_into['expert_table'][e], nll=expert_into['expert_nll'][e])))
                if grouped:
                    expert_into['expert_table'][:, e] += part
                    expert_into['expert_nll'][:, e] += part_nll

    def _confidence_batch(self, batch, temperature, want, threshold, void_label):
        """The routes of _calibrate_batch: where a fused head serves the model ONE ops.fused_head_multi_confidence launch after
        the trunks writes the maps; otherwise the experts' outputs are materialised, fused by the model's own kernel with its
        score output (the mean: its probabilities, kind 1) and handed to ops.confidence_map."""
        from . import ops
        C = self.config['num_classes']
        into = dict(want=want, threshold=threshold, void_label=void_label)
        head = self._agreement_head()
        if head is not None and (fused_head_applicable(self) or multi_head_applicable(self)):
            return ops.fused_head_multi_confidence(*run_lowres_scores_multi(self, batch), C, head[0], temperature, **head[1],
                                                   **into)
        values, kind = self._calibration_values(run_experts(self, batch, self.expert_wants))
        return ops.confidence_map(values.contiguous(), temperature, kind=kind, **into)

    # ---- uncertainty benchmarks of the fused posterior (BaseModel's hooks; csrc/confidence_stats.hip) ----------------------
    def _uncertainty_state(self, batch, experts=False):
        """The routes of _confidence_batch: where a fused head serves the model the trunks stop at their low-resolution scores;
        otherwise the experts' outputs are materialised and fused by the model's own kernel with its score output (the mean:
        its probabilities, kind 1), with every expert's class scores beside them where its own tables are asked for."""
        head = self._agreement_head()
        if head is not None and (fused_head_applicable(self) or multi_head_applicable(self)):
            return {'lowres': run_lowres_scores_multi(self, batch), 'head': head}
        wants = tuple(dict.fromkeys(tuple(self.expert_wants) + (('score',) if experts else ())))
        outs = run_experts(self, batch, wants)
        values, kind = self._calibration_values(outs)
        state = {'values': values.contiguous(), 'kind': kind}
        if experts:
            state['experts'] = [outs[m]['score'].contiguous() for m in self.modalities]
        return state

    def _uncertainty_accumulate(self, state, labels, tables, temperature, fixed_row):
        """ONE ops.fused_head_multi_confidence_stats launch on the low-resolution scores -- the fusion's tables and, asked for,
        every expert's; the materialised state is BaseModel's."""
        if 'lowres' not in state:
            return BaseModel._uncertainty_accumulate(self, state, labels, tables, temperature, fixed_row)
        from . import ops
        m, o = self._uncertainty_bins()
        mode, head_tables = state['head']
        ops.fused_head_multi_confidence_stats(*state['lowres'], self.config['num_classes'], mode, labels, temperature,
                                              fixed_row=fixed_row, mantissa_bits=m, octaves=o,
                                              tables={k: tables[k] for k in ('hist', 'nll', 'counts')},
                                              expert_tables=tables.get('experts'), **head_tables)

    def prediction_difference(self, data):
        """The fused prediction beside every branch's own (dirichlet_mix.py:275-294, uncertainty_dirichlet_mix.py:424-443), as
        numpy arrays: {'fused_label' int64 [N,H,W], 'fused_score' float32 [N,H,W,C], and per modality m '<m>_prob' float32
        [N,H,W,C], '<m>_classification' int64 [N,H,W]}.  The experts' outputs are materialised and fused by the model's own
        fusion kernel.  'fused_score' is there for the models whose fusion has class scores, BayesFusion and DirichletFusion;
        AverageFusion (and any model without `has_fused_score`) omits it.  The MC-dropout fusions draw masks per pass and have
        no fusion of materialised plain outputs: NotImplementedError, as score_agreement."""
        if self.agreement_refusal is not None:
            raise NotImplementedError('%s.prediction_difference: %s' % (type(self).__name__, self.agreement_refusal))
        keys =['fused_label'] + (['fused_score'] if self.has_fused_score else [])
        keys += ['%s_%s' % (m, k) for m in self.modalities for k in ('prob', 'classification')]
        parts = {k: [] for k in keys}
        for batch in self._device_batches(iterate_batches(data, self.config['batchsize']), labels=False):
            for k, v in self._prediction_difference_batch(batch).items():
                parts[k].append(v.cpu().numpy())
        return {k: np.concatenate(v) for k, v in parts.items()}

    def _prediction_difference_batch(self, batch):
        """One batch of prediction_difference, on the device."""
        outs = run_experts(self, batch, ('prob', 'classification'))
        ret = {'fused_label': self._fusion(outs, output_attr=None)}
        if self.has_fused_score:
            ret['fused_score'] = self._fusion(outs, output_attr='fused_score')
        for m in self.modalities:
            ret['%s_prob' % m], ret['%s_classification' % m] = outs[m]['prob'], outs[m]['classification']
        return ret
