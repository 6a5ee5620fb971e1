"""Drop-in mirrors of the tail of ``CalibrationDecoding`` (networks/aoc/decoding_module.py) on the HIP library: ``decoder_final`` (162-190),
``augment_background_logit`` (213-225) and ``predict``, the three lines 144-147 of ``forward`` that turn the decoder's last activation into
the prediction.  They are functions of the decoder object, so they bind onto the reference's class or run on any object
that carries the attributes they read.  The convolutions stay PyTorch modules (MIOpen); everything between them runs in libaoc_hip.so."""
from . import ops


def _gn_relu(bn, x):
    return ops.groupnorm_relu(x, bn.num_groups, bn.weight.detach(), bn.bias.detach(), bn.eps)


def decoder_final(dec, x, low_level_feat, IA_head):
    """decoding_module.py:162-190.  Reads dec.GCT_sc, conv_sc, bn_sc, IA10, conv1, bn1, IA11, conv2, bn2."""
    ops.inference_only("decoder_final", x, low_level_feat, IA_head, dec.IA10.IA.weight, dec.IA11.IA.weight)
    low = _gn_relu(dec.bn_sc, dec.conv_sc(dec.GCT_sc(low_level_feat)))                                  # :165-168
    # :163, :170-176 in one C call: the upsampled tensor and the concatenation are never written ungated
    x = ops.shortcut_stage(x, low, IA_head, dec.IA10.IA.weight.detach(), dec.IA10.IA.bias.detach())
    x = _gn_relu(dec.bn1, dec.conv1(x))                                                                # :177-179
    head = ops.head_delta(IA_head, ops.plane_mean(x))                                                  # :181-183 and the cat of :185
    x = ops.film_scale(x, head, dec.IA11.IA.weight.detach(), dec.IA11.IA.bias.detach())                # :185
    return _gn_relu(dec.bn2, dec.conv2(x))                                                             # :186-188


def augment_background_logit(fg_logit, bg_logit):
    """decoding_module.py:213-225: [N, 1, h, w] x 2 -> [1, N, h, w]."""
    ops.inference_only("augment_background_logit", fg_logit, bg_logit)
    return ops.background_merge(fg_logit, bg_logit)


def predict(dec, x, IA_head):
    """decoding_module.py:144-147: both IA_logit heads and augment_background_logit; x is read once.  -> pred [1, N, h, w]."""
    fg, bg = dec.IA_final_fg, dec.IA_final_bg
    ops.inference_only("predict", x, IA_head, fg.weight, fg.bias, bg.weight, bg.bias)
    wb_fg = ops.linear(IA_head, fg.weight.detach(), fg.bias.detach())                                   # :154, [N, C + 1]
    wb_bg = ops.linear(IA_head, bg.weight.detach(), bg.bias.detach())
    return ops.logit_head(x, wb_fg, wb_bg)
