"""reference: espnet/nets/pytorch_backend/frontends/frontend.py (same class and function names and constructor
arguments, plus beamformer_type ("mvdr", "mpdr" or "wpd"), btaps and bdelay of DNN_Beamformer).  The constructor builds
the beamformer only and still refuses use_wpe=True; WPE dereverberation
(dnn_wpe.py, csrc/wpe.hip) is attached to a built front-end with attach_wpe, after which forward runs the reference's
full logic: in training WPE or the beamformer (never both), in eval WPE and then the beamformer."""
import numpy
import torch

from .dnn_beamformer import DNN_Beamformer
from .dnn_wpe import DNN_WPE


class Frontend(torch.nn.Module):
    def __init__(self, idim, use_wpe=False, wtype="blstmp", wlayers=3, wunits=300, wprojs=320, wdropout_rate=0.0, taps=5,
                 delay=3, use_dnn_mask_for_wpe=True, use_beamformer=False, btype="blstmp", blayers=3, bunits=300, bprojs=320,
                 bnmask=2, badim=320, ref_channel=-1, bdropout_rate=0.0, beamformer_type="mvdr", btaps=5, bdelay=3):
        super().__init__()
        self.use_beamformer = use_beamformer
        self.use_wpe = use_wpe
        self.use_dnn_mask_for_wpe = use_dnn_mask_for_wpe
        self.use_frontend_for_all = bnmask > 2
        if self.use_wpe:
            raise NotImplementedError("WPE dereverberation (use_wpe=True) is not implemented")
        self.wpe = None
        if self.use_beamformer:
            self.beamformer = DNN_Beamformer(btype=btype, bidim=idim, bunits=bunits, bprojs=bprojs, blayers=blayers, bnmask=bnmask,
                                             dropout_rate=bdropout_rate, badim=badim, ref_channel=ref_channel,
                                             beamformer_type=beamformer_type, btaps=btaps, bdelay=bdelay)
        else:
            self.beamformer = None

    def attach_wpe(self, wpe):
        """run `wpe` (a DNN_WPE) as the first stage from now on"""
        if not isinstance(wpe, DNN_WPE):
            raise TypeError(f"attach_wpe takes a DNN_WPE, not {type(wpe).__name__}")
        self.wpe = wpe
        self.use_wpe = True
        return self

    def forward(self, x, ilens):
        """x [B,T,F,2] or [B,T,C,F,2] -> (h, ilens, mask): the beamformer's [B,T,F,2] and speech mask, the dereverberated
        [B,T,C,F,2] and the WPE mask when only WPE ran, or x itself"""
        assert len(x) == len(ilens), (len(x), len(ilens))
        if x.dim() not in (4, 5):
            raise ValueError(f"Input dim must be 4 or 5 with the trailing (re, im) axis: {x.dim()}")
        if not torch.is_tensor(ilens):
            ilens = torch.from_numpy(numpy.asarray(ilens))
        mask = None
        h = x
        if h.dim() == 5:
            if self.training:                       # frontend.py:101-109: the same draw, so a seeded run makes the same choices
                choices = [(False, False)] if not self.use_frontend_for_all else []
                if self.use_wpe:
                    choices.append((True, False))
                if self.use_beamformer:
                    choices.append((False, True))
                use_wpe, use_beamformer = choices[numpy.random.randint(len(choices))]
            else:
                use_wpe, use_beamformer = self.use_wpe, self.use_beamformer
            if use_wpe:
                h, ilens, mask = self.wpe(h, ilens)
            if use_beamformer:
                h, ilens, mask = self.beamformer(h, ilens)
        return h, ilens, mask


def frontend_for(args, idim):
    return Frontend(idim=idim, use_wpe=args.use_wpe, wtype=args.wtype, wlayers=args.wlayers, wunits=args.wunits,
                    wprojs=args.wprojs, wdropout_rate=args.wdropout_rate, taps=args.wpe_taps, delay=args.wpe_delay,
                    use_dnn_mask_for_wpe=args.use_dnn_mask_for_wpe, use_beamformer=args.use_beamformer, btype=args.btype,
                    blayers=args.blayers, bunits=args.bunits, bprojs=args.bprojs, bnmask=args.bnmask, badim=args.badim,
                    ref_channel=args.ref_channel, bdropout_rate=args.bdropout_rate,
                    beamformer_type=getattr(args, "beamformer_type", "mvdr"), btaps=getattr(args, "btaps", 5),
                    bdelay=getattr(args, "bdelay", 3))
