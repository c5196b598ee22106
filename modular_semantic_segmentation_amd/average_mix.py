"""Average fusion (reference: xview/models/average_mix.py)."""
from . import ops
from .basic_fusion_model import FusionModel


class AverageFusion(FusionModel):
    """config: num_units, prefixes, num_channels, expert_model; fused_head=False keeps the experts' probability maps
    materialised (`expert_outputs`) instead of averaging inside the decoder-head kernel."""
    expert_wants = ('prob',)

    def __init__(self, output_dir=None, **config):
        FusionModel.__init__(self, name='AverageFusion', output_dir=output_dir, **config)

    def _fused_head(self):
        return lambda *scores: ops.fused_head_average(*scores, self.config['num_classes'])

    def _multi_head(self):
        return lambda *scores: ops.fused_head_multi(*scores, self.config['num_classes'], 'mean')

    def _agreement_head(self):
        return 'mean', {}

    def _fusion(self, expert_outputs, output_attr=None):
        return ops.average_fuse([expert_outputs[m]['prob'] for m in self.modalities])
