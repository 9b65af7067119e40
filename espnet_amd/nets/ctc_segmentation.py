"""CTC segmentation (Kuerzinger et al. 2020): where the utterances of a transcript start and end in a whole recording, and a
confidence score for each.  The reference (espnet/bin/asr_align.py) leaves this to the external ctc_segmentation package; this
module has that package's call surface (CtcSegmentationParameters, prepare_text, ctc_segmentation,
determine_utterance_segments), so code written against it ports by changing the import, plus a batched form over several
recordings (ctc_segment_batch).  The trellis, the walk back and the segments run on the device (csrc/ctc_segment.hip).

The recursion is the package's, with its windowing, except that unreachable cells are -inf (the package: -1e10, below which fp32
cannot tell two unreachable cells apart) and that the walk back follows stored backpointers (the package re-derives each step
from table differences).  Limits, raised as ValueError before anything is launched: tokens of at most 16 characters, a transcript
no longer than the recording has frames, and a workspace under max_workspace_bytes."""
import numpy as np
import torch

from .. import ops

OK, NO_PATH = 0, 1
DEFAULT_MAX_WORKSPACE_BYTES = 8 << 30


class CtcSegmentationParameters:
    """the package's parameter object: plain attributes, any of them settable through the constructor"""
    min_window_size = 8000
    max_window_size = 100000
    score_min_mean_over_L = 30
    space = "·"
    blank = 0
    replace_spaces_with_blanks = True
    blank_transition_cost_zero = False
    self_transition = "ε"
    start_of_ground_truth = "#"
    excluded_characters = ".,-?!:»«;'›‹()"
    subsampling_factor = 1
    frame_duration_ms = 10
    char_list = None

    def __init__(self, **kwargs):
        for k, v in kwargs.items():
            if not hasattr(type(self), k):
                raise TypeError("unknown segmentation parameter %r" % k)
            setattr(self, k, v)

    @property
    def index_duration_in_seconds(self):
        """seconds per encoder frame"""
        return self.frame_duration_ms * self.subsampling_factor / 1000


def prepare_text(config, text, char_list=None):
    """text: the utterances of one recording, in order -> (ground_truth_mat [L,S] int64, utt_begin_indices [len(text) + 1]).
    The ground truth is "#", then every utterance between space symbols; ground_truth_mat[i, s] is the char_list index of the
    s + 1 characters ending at i (space symbol read as the blank token), -1 where char_list has no such token."""
    if char_list is not None:
        config.char_list = char_list
    chars = list(config.char_list)
    if not 0 <= config.blank < len(chars):
        raise ValueError("blank id %d outside the %d tokens of char_list" % (config.blank, len(chars)))
    blank = chars[config.blank]
    gt = config.start_of_ground_truth
    begins = []
    for utt in text:
        if not gt.endswith(config.space):
            gt += config.space
        begins.append(len(gt) - 1)
        for ch in utt:
            if ch.isspace() and config.replace_spaces_with_blanks:
                if not gt.endswith(config.space):
                    gt += config.space
            elif ch in chars and ch not in config.excluded_characters:
                gt += ch
    if not gt.endswith(config.space):
        gt += config.space
    begins.append(len(gt) - 1)
    S = max(len(c) for c in chars)
    index = {}
    for i, c in enumerate(chars):
        index.setdefault(c, i)
    mat = np.full((len(gt), S), -1, np.int64)
    for i in range(len(gt)):
        for s in range(min(S, i + 1)):
            mat[i, s] = index.get(gt[i - s:i + 1].replace(config.space, blank), -1)
    return mat, np.asarray(begins, np.int64)


def determine_utterance_segments(config, utt_begin_indices, char_probs, timings, text):
    """timings [L] in seconds, char_probs [T] -> [(start, end, confidence)] of every utterance.  Host arithmetic in float64 on
    whatever arrays it is given; ctc_segment_batch computes the same on the device."""
    tm = np.asarray(timings, np.float64)
    cp = np.asarray(char_probs, np.float64)
    idur = config.index_duration_in_seconds
    n = int(config.score_min_mean_over_L)
    segments = []
    for i in range(len(text)):
        b, e = int(utt_begin_indices[i]), int(utt_begin_indices[i + 1])
        start = max(tm[b + 1] - 0.5, (tm[b] + tm[b - 1]) / 2)
        end = min(tm[e - 1] + 0.5, (tm[e] + tm[e - 1]) / 2)
        a, z = int(round(start / idur)), int(round(end / idur))
        if z <= a:
            conf = -np.inf
        elif z - a <= n:
            conf = cp[a:z].mean()
        else:
            csum = np.concatenate(([0.0], np.cumsum(cp[a:z])))
            conf = min(0.0, ((csum[n:-1] - csum[:-n - 1]) / n).min())
        segments.append((float(start), float(end), float(conf)))
    return segments


def format_segments(segment_names, recording_name, segments):
    """the lines of the reference's `segments` file: <segment> <recording> <start> <end> <confidence>"""
    return ["{} {} {:.2f} {:.2f} {:.9f}".format(name, recording_name, s[0], s[1], s[2])
            for name, s in zip(segment_names, segments)]


def _device_of(lpz):
    if isinstance(lpz, torch.Tensor) and lpz.is_cuda:
        return lpz.device
    return torch.device("cuda")


def _plan(config, lens, gts, utts, V, max_workspace_bytes, tmax=None):
    """host checks and the int32 tables of a batch: (tok [B,Umax], gtu [B,Lmax,S], llens, utt [B,NU+1], nutt) as numpy"""
    B = len(gts)
    S = max(g.shape[1] for g in gts)
    if S > ops.CTC_SEGMENT_MAX_S:
        raise ValueError("tokens of %d characters: CTC segmentation takes at most %d" % (S, ops.CTC_SEGMENT_MAX_S))
    if not 0 <= config.blank < V:
        raise ValueError("blank id %d outside the %d outputs" % (config.blank, V))
    for b, g in enumerate(gts):
        if g.shape[0] > lens[b]:
            raise ValueError("Audio is shorter than text (recording %d: %d frames, %d characters)" % (b, lens[b], g.shape[0]))
        if g.shape[0] < 1 or g.max(initial=-1) >= V or g.min(initial=0) < -1:
            raise ValueError("recording %d: ground truth empty or with token ids outside [0, %d)" % (b, V))
    Lmax = max(g.shape[0] for g in gts)
    toks = [[config.blank] + sorted(set(int(v) for v in g[g >= 0].ravel()) - {config.blank}) for g in gts]
    Umax = max(len(t) for t in toks)
    NU = max(1, max(len(u) - 1 for u in utts))
    tok = np.full((B, Umax), -1, np.int32)
    gtu = np.full((B, Lmax, S), -1, np.int32)
    utt = np.zeros((B, NU + 1), np.int32)
    nutt = np.zeros(B, np.int32)
    for b, (g, u) in enumerate(zip(gts, utts)):
        tok[b, :len(toks[b])] = toks[b]
        row = np.full(V + 1, -1, np.int32)
        row[toks[b]] = np.arange(len(toks[b]), dtype=np.int32)
        gtu[b, :g.shape[0], :g.shape[1]] = row[g]                # g == -1 reads row[V] = -1
        u = np.asarray(u, np.int64)
        if u.size >= 2 and (u.min() < 1 or u.max() > g.shape[0] - 1 or np.any(np.diff(u) < 0)):
            raise ValueError("recording %d: utterance begin indices outside the ground truth" % b)
        utt[b, :u.size] = u
        nutt[b] = max(0, u.size - 1)
    llens = np.asarray([g.shape[0] for g in gts], np.int32)
    tmax = max(lens) if tmax is None else tmax
    _check_workspace(B, B, tmax, Lmax, S, Umax, config.min_window_size, max_workspace_bytes)
    return tok, gtu, llens, utt, nutt


def _check_workspace(nsel, B, Tmax, Lmax, S, Umax, window, max_workspace_bytes):
    need = ops.ctc_segment_bytes(nsel, B, Tmax, Lmax, S, Umax, window)
    if need > max_workspace_bytes:
        raise ValueError("CTC segmentation of %d recording(s) at window %d needs %d bytes of workspace (backpointers and "
                         "emission rows), more than max_workspace_bytes = %d" % (nsel, window, need, max_workspace_bytes))


def _segment(config, lpz_pad, lens, gts, utts, max_workspace_bytes, full):
    """the window loop over a batch -> (host results of the last fetch per recording, passes, host reads, windows)"""
    B, Tmax, V = lpz_pad.shape
    lens = [int(v) for v in lens]
    if len(lens) != B or len(gts) != B or min(lens) < 1 or max(lens) > Tmax:
        raise ValueError("lens must give 1 .. %d valid frames for each of the %d recordings" % (Tmax, B))
    tok, gtu, llens, utt, nutt = _plan(config, lens, gts, utts, V, max_workspace_bytes, Tmax)
    dev = _device_of(lpz_pad)
    lpz_pad = torch.as_tensor(lpz_pad).to(device=dev, dtype=torch.float32).contiguous()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tok_d, gtu_d, llens_d, utt_d, nutt_d = up(tok), up(gtu), up(llens), up(utt), up(nutt)
    lens_d = up(np.asarray(lens, np.int32))
    em = ops.ctc_segment_emissions(lpz_pad, lens_d, tok_d, config.blank, config.blank_transition_cost_zero)
    res = ops.ctc_segment_result(B, Tmax, gtu.shape[1], utt.shape[1] - 1, dev)
    window, todo = int(config.min_window_size), list(range(B))
    windows = [window] * B
    passes = reads = 0
    while True:
        ops.ctc_segment_run(em, gtu_d, tok_d, lens_d, llens_d, up(np.asarray(todo, np.int32)), utt_d, nutt_d, res, window,
                            config.score_min_mean_over_L, config.index_duration_in_seconds)
        host = ops.ctc_segment_fetch(res, full)
        passes, reads = passes + 1, reads + 1
        status = host["info"][:, 0]
        if np.any(status[todo] > NO_PATH):
            raise RuntimeError("CTC segmentation failed (status %s)" % status[todo].tolist())
        todo = [b for b in todo if status[b] == NO_PATH]
        if not todo:
            return host, passes, reads, windows
        window *= 2
        if not window < config.max_window_size:
            raise RuntimeError("CTC segmentation: no path for recording(s) %s with windows below max_window_size = %d"
                               % (todo, config.max_window_size))
        for b in todo:
            windows[b] = window
        _check_workspace(len(todo), B, Tmax, gtu.shape[1], gtu.shape[2], tok.shape[1], window, max_workspace_bytes)


def ctc_segmentation(config, lpz, ground_truth_mat, max_workspace_bytes=DEFAULT_MAX_WORKSPACE_BYTES):
    """lpz [T,V] log-probabilities of one recording (numpy or tensor), ground_truth_mat [L,S] from prepare_text
    -> (timings [L] seconds, char_probs [T], state_list [T]: the token string of the frame a character starts at,
    config.self_transition while it lasts, "" off the path)"""
    gt = np.asarray(ground_truth_mat, np.int64)
    lp = lpz if isinstance(lpz, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lpz, dtype=np.float32))
    if lp.dim() != 2 or gt.ndim != 2:
        raise ValueError("lpz must be [T, V] and ground_truth_mat [L, S]")
    L = gt.shape[0]
    utts = [np.asarray([1, L - 1] if L >= 2 else [0])]          # the segments of this call are not returned
    host, _, _, _ = _segment(config, lp.unsqueeze(0), [lp.shape[0]], [gt], utts, max_workspace_bytes, True)
    chars = list(config.char_list) if config.char_list is not None else None
    names = {-1: config.self_transition, -2: ""}
    state_list = [names[s] if s < 0 else (chars[s] if chars is not None else str(s)) for s in host["states"][0].tolist()]
    timings = host["timings"][0].astype(np.float64) * config.index_duration_in_seconds
    return timings, host["char_probs"][0].copy(), state_list


def ctc_segment_batch(config, lpz_pad, lens, texts, max_workspace_bytes=DEFAULT_MAX_WORKSPACE_BYTES):
    """lpz_pad [B,Tmax,V] log-probabilities (rows behind lens[b] are never read), texts[b]: the utterances of recording b
    -> per recording the list of (start, end, confidence), seconds.  Every recording starts at config.min_window_size; those
    without a path in their window are run again together at twice the size, the others keep their result.  One
    device-to-host copy per window attempt.  ctc_segment_batch.passes / .host_reads / .windows: attempts, copies and the final
    window of each recording of the last call."""
    prepared = [prepare_text(config, t) for t in texts]
    host, passes, reads, windows = _segment(config, lpz_pad, lens, [p[0] for p in prepared], [p[1] for p in prepared],
                                            max_workspace_bytes, False)
    ctc_segment_batch.passes, ctc_segment_batch.host_reads, ctc_segment_batch.windows = passes, reads, windows
    return [[tuple(float(v) for v in host["seg"][b, i]) for i in range(len(texts[b]))] for b in range(len(texts))]


ctc_segment_batch.passes = ctc_segment_batch.host_reads = 0
ctc_segment_batch.windows = []
