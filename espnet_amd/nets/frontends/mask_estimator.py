"""BLSTMP mask estimator.  reference: espnet/nets/pytorch_backend/frontends/mask_estimator.py (same class name,
constructor arguments and parameter names)."""
import numpy as np
import torch

from ... import functional as F_
from ..rnn.encoders import RNN, RNNP


class MaskEstimator(torch.nn.Module):
    def __init__(self, type, idim, layers, units, projs, dropout, nmask=1):
        super().__init__()
        subsample = np.ones(layers + 1, dtype=np.int64)
        typ = type.lstrip("vgg").rstrip("p")
        if type[-1] == "p":
            self.brnn = RNNP(idim, layers, units, projs, subsample, dropout, typ=typ)
        else:
            self.brnn = RNN(idim, layers, units, projs, dropout, typ=typ)
        self.type = type
        self.nmask = nmask
        self.linears = torch.nn.ModuleList([torch.nn.Linear(projs, idim) for _ in range(nmask)])

    def logits(self, xs, ilens):
        """xs [B,T,C,F,2] spectrum, ilens [B] -> mask logits [nmask, B, C, Tm, F], Tm = max(ilens): the layout in which
        the Linear layers produce them and eamd_bf_psd reads them.  The magnitude spectrum enters as data (the
        spectrum carries no gradient)."""
        B, T, C, F, _ = xs.shape
        ilens = [int(v) for v in ilens]
        assert len(ilens) == B, (B, len(ilens))
        with torch.no_grad():
            mag = torch.linalg.vector_norm(xs, dim=-1).transpose(1, 2).reshape(B * C, T, F)   # (B*C, T, F)
        ilens_ = [v for v in ilens for _ in range(C)]
        hs, _, _ = self.brnn(mag, ilens_)                                                     # (B*C, Tm, projs)
        Tm = hs.shape[1]
        return torch.stack([F_.LinearFn.apply(hs, lin.weight, lin.bias).view(B, C, Tm, F) for lin in self.linears])

    @staticmethod
    def masks_from_logits(logits, input_length):
        """[nmask,B,C,Tm,F] -> tuple of the reference's masks (B, F, C, T), zero for Tm <= t < T
        (mask_estimator.py:65-75; frames between an utterance's length and Tm keep sigmoid(bias), :67)"""
        masks = torch.sigmoid(logits).permute(0, 1, 4, 2, 3)
        if masks.size(-1) < input_length:
            masks = torch.nn.functional.pad(masks, [0, input_length - masks.size(-1)], value=0)
        return tuple(masks.unbind(0))

    def forward(self, xs, ilens):
        """xs [B,T,C,F,2], ilens [B] -> (masks: nmask tensors (B, F, C, T), ilens)"""
        return self.masks_from_logits(self.logits(xs, ilens), xs.shape[1]), ilens
