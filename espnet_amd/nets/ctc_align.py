"""CTC forced alignment of a padded batch through a whole model: the batch branch of the reference's forced alignment
(ctc.py:153-216 raises NotImplementedError("Align_batch is not implemented.")) and the model side of its ctc_align stage
(asr/pytorch_backend/asr.py:1368-1446, which aligns one utterance per call).  No JSON / CLI work here."""
import torch

from .. import ops
from .modules import embed_output_lengths, make_non_pad_mask, subsampled_stride


def _lengths(ilens):
    return [int(v) for v in (ilens.tolist() if isinstance(ilens, torch.Tensor) else ilens)]


def encode_batch(model, xs_pad, ilens, alone=False):
    """the model's encoder on a padded batch in one call, in eval mode (the model's train / eval mode is restored after)
    -> (hs_pad (B,T',D), hlens list of valid encoder frames).  espnet2 ESPnetASRModel: encode(speech, lengths); espnet1 RNN E2E:
    enc(xs_pad, ilens); espnet1 Transformer / Conformer E2E: encoder(xs_pad, mask).  As in the reference's batches, the valid
    frames of a padded utterance are those of the subsampled mask (one more than the same utterance gets unpadded behind a conv2d
    input layer), and layers without a mask (the Conformer convolution module) see the padding of the shorter utterances: a
    padded utterance's encoder output, and so its alignment, can differ from the one it has alone.
    alone=True (espnet1 Transformer / Conformer): every utterance keeps the encoder frames it has alone, and the encoder mask is
    the one model.prepare(pad_to=) builds for them; a Transformer encoder then gives each utterance the output it has alone."""
    from ..espnet2.asr import ESPnetASRModel
    dev = next(model.parameters()).device
    il = _lengths(ilens)
    xs_pad = torch.as_tensor(xs_pad, dtype=torch.float32).to(dev)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            if isinstance(model, ESPnetASRModel):
                hs_pad, hlens = model.encode(xs_pad, torch.as_tensor(il, dtype=torch.int64))
                return hs_pad, _lengths(hlens)
            if hasattr(model, "enc"):                                             # espnet1 RNN
                ops.zero_arena_off()
                hs_pad, hlens, _ = model.enc(xs_pad, il)
                return hs_pad, _lengths(hlens)
            if hasattr(model, "encoder"):                                         # espnet1 Transformer / Conformer
                tmax = max(il)
                xs_pad = xs_pad[:, :tmax].contiguous()
                mask_len = il
                if alone:
                    hl = [embed_output_lengths(model.encoder.embed, [n], n)[0] for n in il]
                    stride = max(1, subsampled_stride(model.encoder.embed))
                    mask_len = [(h - 1) * stride + 1 if h > 0 else 0 for h in hl]
                mask = make_non_pad_mask(mask_len, tmax).unsqueeze(-2).to(torch.uint8).to(dev)
                ops.zero_arena_off()
                hs_pad, _ = model.encoder(xs_pad, mask)
                return hs_pad, hl if alone else embed_output_lengths(model.encoder.embed, il, tmax)
    finally:
        model.train(was_training)
    raise TypeError("%s has no encoder this helper knows" % type(model).__name__)


def ctc_align_batch(model, xs_pad, ilens, ys_pad, blank_id=0):
    """xs_pad (B,T,idim) features, ilens (B) valid frames, ys_pad (B,L) label ids padded with -1 -> modules.CTCAlignment of
    the encoder frames (score, states, tokens, start, end; device tensors): one encoder call, one alignment pass"""
    hs_pad, hlens = encode_batch(model, xs_pad, ilens)
    return model.ctc.forced_align_batch(hs_pad, hlens, ys_pad, blank_id)


def ctc_segment_recordings(model, xs_pad, ilens, texts, config, **kw):
    """xs_pad (B,T,idim) features of whole recordings, ilens (B) valid frames, texts[b] the utterances of recording b, config a
    ctc_segmentation.CtcSegmentationParameters (char_list; subsampling_factor = the encoder's frame rate reduction) -> per
    recording the list of (start, end, confidence) in seconds (the model side of the reference's bin/asr_align.py, which
    segments one recording per call): one encoder call, then CTC.segment"""
    hs_pad, hlens = encode_batch(model, xs_pad, ilens)
    return model.ctc.segment(hs_pad, hlens, texts, config, **kw)
