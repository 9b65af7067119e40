"""Speech-enhancement front-end of the reference (espnet/nets/pytorch_backend/frontends/*): the mask-based MVDR
beamformer on the espnet_amd HIP kernels (csrc/beamformer.hip).  WPE dereverberation is not on this path."""
