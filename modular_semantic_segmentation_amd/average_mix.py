"""Average fusion (reference: xview/models/average_mix.py)."""
import torch

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

    def _calibration_values(self, expert_outputs):
        # the mean probabilities average_fuse decides by: ((p_0 + p_1) + ...) / E, the division by a device tensor so that it
        # is an IEEE division per element, as the kernels divide (a host scalar would become a product with 1 / E)
        probs = [expert_outputs[m]['prob'] for m in self.modalities]
        total = probs[0]
        for p in probs[1:]:
            total = total + p
        return total / torch.tensor(float(len(probs)), dtype=torch.float32, device=total.device), 1

    def _fusion(self, expert_outputs, output_attr=None):
        return ops.average_fuse([expert_outputs[m]['prob'] for m in self.modalities])
