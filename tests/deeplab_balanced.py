"""Test helper: a synthetic DeepLab net whose class maps are not one class.

The seeded nets (deeplab_spec.build_deeplab) draw their logits layer at random: on most frames one class
wins everywhere, and a test of the class-map path on such a map would pass with the LUT's single entry
and nothing else right. balance_logits shifts the logits bias by each class's own mean logit over a probe
batch (one fp32 forward on the GPU), so every class wins somewhere and the argmax is decided by the
spatial variation of the features."""
import numpy as np

from bugcar_image_segmentation_amd.models import DeepLabV3


def balance_logits(net, probe_frames):
    """net with its logits bias re-centred on probe_frames ((B, H, W, 3) u8 RGB); changes net in place."""
    model = DeepLabV3(net=net, precision="fp32")
    model.predict(probe_frames)
    lg = model.logits_device().cpu().numpy()[..., :net.num_classes]
    mean = lg.reshape(-1, net.num_classes).mean(0)
    net.logits.b = (net.logits.b - mean).astype(np.float32)
    return net
