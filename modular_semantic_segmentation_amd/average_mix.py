"""Average fusion (reference: xview/models/average_mix.py)."""
from . import ops
from .basic_fusion_model import FusionModel, fused_head_applicable, run_lowres_scores


class AverageFusion(FusionModel):
    """config: num_units, prefixes, num_channels, expert_model; fused_head=False keeps the experts' probability maps
    materialised (`expert_outputs`) instead of averaging inside the decoder-head kernel."""
    expert_wants = ('prob',)

    def __init__(self, output_dir=None, **config):
        FusionModel.__init__(self, name='AverageFusion', output_dir=output_dir, **config)

    def _predict_batch_impl(self, batch, output_attr=None):
        if output_attr is None and fused_head_applicable(self):
            # default prediction: the experts' probabilities never leave the registers of the fused average head
            self.expert_outputs = None
            Sa, Sb, ba, bb, n, hi, wi = run_lowres_scores(self, batch)
            return ops.fused_head_average(Sa, Sb, ba, bb, n, hi, wi, self.config['num_classes'])
        return FusionModel._predict_batch_impl(self, batch, output_attr)

    def _fusion(self, expert_outputs, output_attr=None):
        return ops.average_fuse([expert_outputs[m]['prob'] for m in self.modalities])
