"""Transducer decoding on the device primitives: greedy search, the default (Graves) beam search, tsd, alsd and nsc.

What the searches compute is pinned by the reference (espnet/nets/beam_search_transducer.py:130-237: one symbol per
frame at most in the greedy search; the A / B hypothesis sets of Graves 2012 in the default search, RNNLM shallow
fusion added to the non-blank extensions) and by the recorded hypotheses in tests/golden/transducer_*.npz.  How it is
computed is this package's own design:

  * label prefixes live in a TRIE (`_Prefixes`): a hypothesis is (score, node).  Everything that depends on the
    label sequence only - the prediction network's output and state, the LM state and scores - is stored ONCE per
    node under its integer id, so two hypotheses that reach the same sequence share it;
  * the joint network runs on ROWS: `JointNetwork.joint_rows` takes n (frame, node) pairs and returns n log-softmax
    rows from one lin_dec GEMM, one fused add + activation, one lin_out GEMM and one log-softmax launch;
  * greedy search: the prediction output only changes when a symbol is emitted, so a whole CHUNK of frames is scored
    against the current node in one batch, the first non-blank frame is located on the device and only that index
    and token come back to the host - launches scale with emitted symbols, not with frames;
  * batched greedy search (`greedy_batch`): all utterances of a batch frame by frame in lock-step - a fused joint + argmax
    launch that never stores the logits, a bookkeeping launch, a masked prediction-network step - with no host read inside the
    frame loop and one at the end, optionally as replays of one captured frame step;
  * default beam search: at the start of a frame all carried hypotheses are scored in one batch (prediction steps for
    nodes first seen + joint rows + top-k, one device-to-host copy); children created during the frame are scored
    lazily, again all pending ones in one batch, when the first of them is selected for expansion.

  * time-synchronous (tsd), alignment-length-synchronous (alsd) and N-step-constrained (nsc) searches (reference:
    :239-663): every PASS scores all pending (encoder row, node) pairs in one joint_rows call, and one
    transducer_expand_rows launch hands the host what the pass needs - blank log-probability, the k best non-blank
    (log-probability, token) pairs, the LM log-probability of each chosen token, nsc's prefix-rescoring terms - through
    ONE blocking device-to-host copy (`_expand`, counted in `host_reads`);
  * batched alsd (`alsd_batch`): the alsd search of all utterances of a batch step by step in lock-step, hypotheses in device
    arrays instead of the trie, the beam bookkeeping of a step in one launch (eamd_rnnt_alsd_step), no host read inside the step
    loop and one at the end;
  * batched tsd (`tsd_batch`): the tsd search of all utterances of a batch pass by pass in lock-step, hypotheses in M + 1 device
    blocks (B's two parities and the C of every pass), the A / C / B bookkeeping of a pass in one launch (eamd_rnnt_tsd_step), no
    host read inside the pass loop and one at the end;
  * RNN LM shallow fusion in alsd_batch / tsd_batch (lm=ClassifierWithState(RNNLM), lm_batched=True; `_lm_batched_ok`.  The switch
    is off by default: with an LM both calls looped over the per-utterance search before, and they keep doing so unless asked):
    in these two searches the LM
    advances exactly when the prediction network does, so its h / c ride in the same state copies / blocks, move in the same
    eamd_gather_rows launch and step through the same masked cell kernels (`_stack_step`); its log-probabilities of all rows of a
    pass come from the top layer's h (lo + log-softmax), eamd_transducer_expand_rows picks the chosen tokens' terms into its
    record on the device, and eamd_rnnt_alsd_step_lm / eamd_rnnt_tsd_step_lm add them with the reference's float32 arithmetic
    (below).  nsc_batch and default_batch keep looping over the per-utterance search when an LM is given: there the LM's scores
    travel with the hypothesis (nsc) or the LM steps at pop time (default), which takes other loops;
  * batched nsc (`nsc_batch`): the nsc search of all utterances of a batch n-step by n-step in lock-step, hypotheses in N + 2 device
    blocks (kept's two parities and the V of every n-step), prefix rescoring, S, substract and the selections of a call in one
    launch (eamd_rnnt_nsc_step), the rescoring's pair terms from a device-side pair list, no host read inside the frame loop and
    one at the end;
  * batched default (`default_batch`): the default search of all utterances of a batch POP by pop in lock-step, every utterance
    with its own frame counter on the device; A (sorted, cut to default_max_pops entries) and B in device arrays, the
    prediction-network states in a pool of two frame-parity regions, labels as a log of (parent, token) records; finishing a pop,
    ending a frame and selecting the next pop in one launch (eamd_rnnt_default_step); the host reads the done flags after the
    first beam x frames steps and after every further chunk, then ONE result copy; an utterance whose frame wants more pops than
    default_max_pops (an untrained, flat model does) overflows and is searched again per utterance;
  * what the five batched searches share is written once, above them: the loop over the per-utterance search for a batch the device
    loops do not take (`_fallback` over `_one`), the lengths (`_lengths`), encoder projection + chunking by *_max_rows + the call's one
    result copy (`_chunks`), one result layout per search from which the buffer is both built and taken apart (`_pack` / `_unpack`),
    the n-best order (`_nbest`), the masked cell-stack step the prediction network and the RNN LM both run (`_stack_step`) and the
    scratch builders (`_pred_ws`, `_block_ws`, `_lm_ws`, `_frame_rows`); the five step loops differ for
    real and stay apart.  On the device the same holds for rnnt_search.h (score key, stable rank, label comparison and copy) and
    row_moves.hip (eamd_gather_rows / eamd_scatter_rows).

Prediction networks take part through one of three protocols: `step(tokens, states)` (batched; DecoderRNNT),
`batch_step(yseqs)` (DecoderTT: the reference's batch_score, whose outputs depend on the batch a prefix is first computed
in - the searches call it with the reference's hypothesis lists, in the reference's order) or the reference's
per-hypothesis plug-in method `score(hyp, cache, init_tensor)` (any TransducerDecoderInterface; greedy and default only).

tsd / alsd / nsc reproduce the reference as recorded in the fixtures, its quirks included: tsd's last symbol expansion
still scores and expands (`v < max_sym_exp` always holds); alsd never scores frame 0, `recombine_hyps` returns its input
(duplicates stay, the first occurrence's score grows in place) and B is returned unsorted when no hypothesis reached the
last frame; nsc's prefix rescoring mutates scores in length order and adds the last step's blank only when nstep != 1.
Once an LM term is added, tsd / alsd scores are float32 0-d tensors in the reference (score + lm_weight * tensor): they are
carried the same way here, by the per-utterance searches as tensors and by the device loops as doubles that hold float32 values
(every sum, the LM product and the logaddexp of a merge rounded to float32 from the first label on; [blank] and its blank
continuations stay double; the n-best sort divides in float32).  One reference behaviour is NOT copied: its prediction / LM
caches are keyed by "".join(str(x) for x in yseq), which collides once V > 10 ([1, 23] and [12, 3]); the trie's node ids do not."""
import math
from dataclasses import dataclass, field
from typing import Any, List

import numpy as np
import torch

from .. import ops


@dataclass
class Hypothesis:
    """result record (the fields the reference's recognisers read: score, yseq; the state fields stay empty)"""

    score: float
    yseq: List[int]
    dec_state: Any = None
    lm_state: Any = None
    y: Any = None
    lm_scores: Any = None


class _Prefixes:
    """trie of label sequences; node 0 = [blank]"""

    def __init__(self, blank):
        self.parent, self.token, self.kids = [-1], [blank], [{}]

    def child(self, node, tok):
        c = self.kids[node].get(tok)
        if c is None:
            c = len(self.parent)
            self.parent.append(node)
            self.token.append(tok)
            self.kids.append({})
            self.kids[node][tok] = c
        return c

    def labels(self, node):
        out = []
        while node >= 0:
            out.append(self.token[node])
            node = self.parent[node]
        return out[::-1]


@dataclass
class _View:
    """what a TransducerDecoderInterface.score() reads of a hypothesis"""

    yseq: List[int]
    dec_state: Any
    score: float = 0.0
    lm_state: Any = None


@dataclass
class _Pred:
    """per-node results of the prediction network (and of the LM, filled on first expansion)"""

    out: dict = field(default_factory=dict)       # node -> (dunits,) output
    state: dict = field(default_factory=dict)     # node -> state AFTER consuming the node's token
    lm_state: dict = field(default_factory=dict)
    lm_logp: dict = field(default_factory=dict)   # node -> host list of LM log-probabilities of the next token
    lm_dev: dict = field(default_factory=dict)    # node -> (device [m, V] LM log-probabilities, row): tsd / alsd / nsc


_SEARCHES = {"default": "_default", "tsd": "_tsd", "alsd": "_alsd", "nsc": "_nsc"}

# ---- result layouts -------------------------------------------------------------------------------------------------------
# A batched search hands its results to the host in ONE int32 buffer.  What is in it is said once, by a layout: an ordered list of
# (name, shape, numpy dtype) with int32 / float32 fields taking one word per element and float64 fields two.  `_pack` builds the
# buffer on the device from it, `_unpack` takes the host copy apart by it.
_TORCH = {np.int32: torch.int32, np.float32: torch.float32, np.float64: torch.float64}


def _fields(layout, o=0):
    """(name, shape, dtype, first word, words) of every field of a layout that starts at word o"""
    for name, shape, dt in layout:
        words = int(np.prod(shape, dtype=np.int64)) * (np.dtype(dt).itemsize // 4)
        yield name, shape, dt, o, words
        o += words


def _pack(layout, tensors):
    """the layout's fields, given in its order as tensors (float fields contiguous), as one int32 buffer"""
    parts = []
    for (name, shape, dt), x in zip(layout, tensors):
        assert tuple(x.shape) == tuple(shape) and x.dtype == _TORCH[dt], name
        parts.append((x if dt is np.int32 else x.view(torch.int32)).reshape(-1))
    return torch.cat(parts)


def _unpack(layout, words, o=0):
    """words: int32 numpy array that holds a packed layout from word o on -> ({name: array}, the first word after it)"""
    out = {}
    for name, shape, dt, first, n in _fields(layout, o):
        a = words[first:first + n]
        out[name] = (a if dt is np.int32 else a.copy().view(dt)).reshape(shape)      # the copy aligns a float64 field
        o = first + n
    return out, o


class _Hyp:
    """a hypothesis of the tsd / alsd / nsc searches: mutable score (the reference updates scores in place) + trie node"""

    __slots__ = ("score", "node")

    def __init__(self, score, node):
        self.score, self.node = score, node


class BeamSearchTransducer:
    def __init__(self, decoder, beam_size, lm=None, lm_weight=0.1, search_type="default", max_sym_exp=2, u_max=50,
                 nstep=1, prefix_alpha=1, score_norm=True, frame_chunk=32, lm_batched=False):
        self.decoder = decoder
        self.beam_size = beam_size
        self.vocab_size = decoder.odim
        self.blank = decoder.blank
        if self.blank != 0:
            raise NotImplementedError("blank id must be 0 (the non-blank top-k is taken over ids 1..V-1)")
        self.batched = hasattr(decoder, "step")
        if beam_size > 1 and search_type not in _SEARCHES:
            raise NotImplementedError("search_type %r: one of %s" % (search_type, ", ".join(_SEARCHES)))
        if beam_size > 1 and search_type != "default" and not (self.batched or hasattr(decoder, "batch_step")):
            raise NotImplementedError("search_type %r needs a prediction network with a batched step (step or batch_step)"
                                      % search_type)
        self.search_type = search_type
        self.lm, self.lm_weight = lm, lm_weight
        self.lm_batched = lm_batched           # alsd_batch / tsd_batch take an RNN LM into their device loops (_lm_batched_ok)
        self.max_sym_exp, self.u_max, self.nstep, self.prefix_alpha = max_sym_exp, u_max, nstep, prefix_alpha
        self.score_norm = score_norm
        self.frame_chunk = frame_chunk
        self.passes = self.host_reads = 0      # tsd / alsd / nsc: search passes and blocking host reads of the last call

    @ops.inference_call
    def __call__(self, h):
        """h: encoder states of one utterance (T, D_enc) -> 1-best Hypothesis (greedy) or the sorted n-best list"""
        if hasattr(self.decoder, "att"):          # rnnt-att: forget the previous utterance's encoder projections
            self.decoder.att[0].reset()
        with torch.no_grad():
            if self.beam_size <= 1:
                return self._greedy(h)
            return getattr(self, _SEARCHES[self.search_type])(h)

    # ---- prediction network, once per trie node ---------------------------------------------------------------------
    def _start(self, h):
        self._tree = _Prefixes(self.blank)
        self._pred = _Pred()
        self._init_tensor = h.unsqueeze(0)
        self._root_state = self.decoder.init_state(self._init_tensor)
        self._ext_cache = {}

    def _ensure_pred(self, nodes):
        """prediction-network output / state for every node of `nodes` that has none yet (parents always have)"""
        todo = [n for n in dict.fromkeys(nodes) if n not in self._pred.out]
        if not todo:
            return
        tr, pr, dec = self._tree, self._pred, self.decoder
        if self.batched:
            dev = self._init_tensor.device
            toks = torch.tensor([tr.token[n] for n in todo], dtype=torch.long, device=dev)
            prev = [pr.state[tr.parent[n]] if tr.parent[n] >= 0 else dec.unbatch_state(self._root_state, 0) for n in todo]
            y, new = dec.step(toks, dec.batch_states(prev))
            for i, n in enumerate(todo):
                pr.out[n] = y[i]
                pr.state[n] = dec.unbatch_state(new, i)
        else:
            for n in todo:
                prev = pr.state[tr.parent[n]] if tr.parent[n] >= 0 else self._root_state
                y, st, _ = dec.score(_View(tr.labels(n), prev), self._ext_cache, self._init_tensor)
                pr.out[n] = y.reshape(-1)
                pr.state[n] = st

    def _lm_step(self, node):
        """LM log-probabilities of the token after `node` (RNNLM shallow fusion), once per node"""
        pr = self._pred
        if node not in pr.lm_logp:
            par = self._tree.parent[node]
            prev = pr.lm_state[par] if par >= 0 else None
            tok = torch.tensor([self._tree.token[node]], dtype=torch.long, device=self._init_tensor.device)
            st, logp = self.lm.predict(prev, tok)
            pr.lm_state[node] = st
            pr.lm_logp[node] = logp[0].tolist()
        return pr.lm_logp[node]

    def _rows(self, enc_rows, nodes):
        """log-softmax rows of the joint network for n (encoder row, node) pairs -> (n, V)"""
        y = torch.stack([self._pred.out[n] for n in nodes])
        return ops.log_softmax_rows(self.decoder.joint_network.joint_rows(enc_rows, y))

    # ---- greedy -----------------------------------------------------------------------------------------------------
    def _greedy(self, h):
        self._start(h)
        jn = self.decoder.joint_network
        enc = jn.project_enc(h)
        T = enc.shape[0]
        node, score, t = 0, 0.0, 0
        self._ensure_pred([0])
        while t < T:
            n = min(self.frame_chunk, T - t)
            logp = ops.log_softmax_rows(jn.joint_rows(enc[t:t + n], self._pred.out[node].unsqueeze(0)))
            best = ops.argmax_rows(logp).long()                                     # (n,)
            emit = (best != self.blank)
            # first emitting frame of the chunk, its token and log-probability: one small copy to the host
            first = torch.where(emit, torch.arange(n, device=best.device), torch.full((), n, device=best.device)).min()
            idx = first.clamp(max=n - 1)
            rec = torch.stack([first.float(), best[idx].float(), logp[idx, best[idx]]]).tolist()
            f = int(rec[0])
            if f >= n:                     # only blanks in this chunk
                t += n
                continue
            node = self._tree.child(node, int(rec[1]))
            score += rec[2]
            self._ensure_pred([node])
            t += f + 1                     # at most one symbol per frame (reference greedy_search)
        return Hypothesis(score=score, yseq=self._tree.labels(node))

    # ---- batched searches: what all five share --------------------------------------------------------------------------
    def _one(self, name, h):
        """the per-utterance search `name` (looked up on self at call time) on one row of a batch"""
        if hasattr(self.decoder, "att"):
            self.decoder.att[0].reset()
        with torch.no_grad():
            return getattr(self, name)(h)

    def _fallback(self, name, hs_pad, hlens):
        """a batch the device loops do not take: a loop over the per-utterance search"""
        B, T = hs_pad.shape[:2]
        if hlens is None:
            lens = [T] * B
        else:
            lens = [int(v) for v in (hlens.tolist() if torch.is_tensor(hlens) else hlens)]
        return [self._one(name, hs_pad[b, :lens[b]]) for b in range(B)]

    @staticmethod
    def _lengths(hlens, B, T, dev):
        """hlens (None / list / tensor) -> (frames per utterance on the host, the same as a device int32 vector), both in [0, T].
        A device tensor is not read: its host list is [T] * B, the padded length, which only bounds the loops."""
        # The clamp is every caller's: the kernels take T_b = max(0, min(hlens[b], T)) themselves, the host's (hl - 1).clamp(0, 1)
        # and minimum(t, hl - 1).clamp_(min=0) give 0 for any length <= 0, and a loop length is a maximum over a chunk of frames,
        # W * frames or alsd's t + min(u_max, t - 1) (<= -1 for t <= 0, clamped or not): a length <= 0 never sets it.
        if hlens is None or torch.is_tensor(hlens):
            frames = [T] * B
            hl = (torch.full((B,), T, dtype=torch.int32, device=dev) if hlens is None
                  else hlens.to(device=dev, dtype=torch.int32).clamp(min=0, max=T))
        else:
            frames = [max(0, min(int(v), T)) for v in hlens]
            hl = torch.tensor(frames, dtype=torch.int32).to(dev, non_blocking=True)
        return frames, hl

    def _chunks(self, hs_pad, nmax, rows):
        """projects the encoder, runs rows(enc [B, T, J], b0, b1) -> (result buffer, its layout) on every chunk of nmax
        utterances and reads all the buffers in the call's ONE blocking copy -> per chunk the layout's {name: host array}"""
        B, T = hs_pad.shape[:2]
        enc = self.decoder.joint_network.project_enc(hs_pad.reshape(B * T, -1)).view(B, T, -1)
        res = [rows(enc, b0, min(B, b0 + nmax)) for b0 in range(0, B, nmax)]
        host = (res[0][0] if len(res) == 1 else torch.cat([r[0] for r in res])).cpu().numpy()
        out, o = [], 0
        for _buf, layout in res:
            got, o = _unpack(layout, host, o)
            out.append(got)
        return out

    def _nbest(self, hyps, length=lambda x: len(x.yseq)):
        """the reference's n-best order: score / length descending (score with score_norm=False), equal keys in list order"""
        if self.score_norm:
            return sorted(hyps, key=lambda x: x.score / length(x), reverse=True)
        return sorted(hyps, key=lambda x: x.score, reverse=True)

    def _pred_ws(self, R, dev, copies=2):
        """what _pred_step needs on R rows besides lin_dec's output `d`: the token and mask vectors (zero: nothing emitted),
        `copies` copies of the prediction network's state (zero) and the step's intermediates"""
        dec = self.decoder
        ws = dict(n=R)
        ws["tok"] = torch.zeros(R, device=dev, dtype=torch.int64)
        ws["live"] = torch.zeros(R, device=dev, dtype=torch.uint8)
        ws.update(self._stack_ws(R, dec.dunits, dec.dlayers, dec.dtype, dev, copies))
        return ws

    @staticmethod
    def _stack_ws(R, H, L, typ, dev, copies):
        """what _stack_step needs on R rows of an L-layer cell stack of H units besides the token and mask vectors: `copies` copies
        of its state (zero) and the step's intermediates"""
        G = (4 if typ == "lstm" else 3) * H
        f = dict(device=dev, dtype=torch.float32)
        ws = {}
        ws["h"] = [[torch.zeros(R, H, **f) for _ in range(L)] for _ in range(copies)]
        ws["c"] = [[torch.zeros(R, H, **f) for _ in range(L)] for _ in range(copies)]
        ws["gx"] = [torch.empty(R, G, **f) for _ in range(L)]
        ws["gates"] = [torch.empty(R, 4 * H, **f) for _ in range(L)]       # lstm: pre-activations / activated gates; gru: acts
        ws["gh"] = [torch.empty(R, G, **f) for _ in range(L)] if typ == "gru" else None
        return ws

    @staticmethod
    def _stack_blocks(ws, blocks, R, H, dev, **extra):
        """ws (one state copy) -> the state of `blocks` blocks of R rows stacked [blocks * R, H] per layer in ws["h"] / ws["c"], the
        copy ws had as the staging copy, and the list of per-block views: state copy 0 = the staging copy, copy 1 = the block's
        rows, plus extra[name][j] under `name`"""
        stage_h, stage_c = ws["h"][0], ws["c"][0]
        ws["h"] = [torch.zeros(blocks * R, H, device=dev, dtype=torch.float32) for _ in stage_h]
        ws["c"] = [torch.zeros(blocks * R, H, device=dev, dtype=torch.float32) for _ in stage_c]
        return [dict(ws, h=[stage_h, [x[j * R:(j + 1) * R] for x in ws["h"]]],
                     c=[stage_c, [x[j * R:(j + 1) * R] for x in ws["c"]]], **{name: v[j] for name, v in extra.items()})
                for j in range(blocks)]

    def _lm_ws(self, R, tok, dev, blocks=0):
        """the LM's side of a device loop on R rows: the state of its cell stack as _pred_ws keeps the prediction network's (two
        copies, or with `blocks` the stacked blocks and a staging copy of _block_ws, views under "blk"), the step's intermediates, the
        loop's token vector `tok`, the [R, V] buffers of the LM's output rows ("z": logits; "logp": the log-probabilities of the
        last pass that computed them, zero before) and the device iota eamd_transducer_expand_rows takes as lm_row"""
        net = self.lm.predictor
        ws = dict(n=R, tok=tok)
        ws.update(self._stack_ws(R, net.n_units, net.n_layers, net.typ, dev, 1 if blocks else 2))
        ws["z"] = torch.empty(R, self.vocab_size, device=dev, dtype=torch.float32)
        ws["logp"] = torch.zeros(R, self.vocab_size, device=dev, dtype=torch.float32)
        ws["iota"] = torch.arange(R, device=dev, dtype=torch.int32)
        if blocks:
            ws["blk"] = self._stack_blocks(ws, blocks, R, net.n_units, dev)
        return ws

    def _block_ws(self, blocks, R, d, dev):
        """tsd / nsc: the prediction network's state of `blocks` hypothesis blocks of R rows stacked [blocks * R, H] per layer (a
        block row indexes it directly), one staging copy, and ws["blk"][j] = _pred_step's view of block j: state copy 0 = the
        staging copy, copy 1 = the block's rows, d = d[j]"""
        ws = self._pred_ws(R, dev, copies=1)
        ws["blk"] = self._stack_blocks(ws, blocks, R, self.decoder.dunits, dev, d=d)
        return ws

    @staticmethod
    def _frame_rows(hl, T, W, frames, levels=1):
        """tsd / nsc: [frames, levels * n * W] int32, the encoder row of frame t for every row of a block, b * T + min(t, T_b - 1):
        the same for all slots of an utterance and for each of `levels` stacked copies of the block"""
        n, dev = hl.shape[0], hl.device
        tt = torch.arange(frames, device=dev, dtype=torch.int32)
        ft = torch.minimum(tt[:, None], (hl - 1)[None, :]).clamp_(min=0) + (torch.arange(n, device=dev, dtype=torch.int32) * T)
        ft = ft.repeat_interleave(W, dim=1)
        return (ft.repeat(1, levels) if levels > 1 else ft).contiguous()

    # ---- batched greedy ---------------------------------------------------------------------------------------------
    # The reference's greedy search emits at most one symbol per frame, so the utterances of a batch advance through the frames in
    # lock-step: frame t of all rows is one fused joint + argmax launch (eamd_rnnt_greedy_joint: the [B, V] logits are never stored),
    # one bookkeeping launch (eamd_rnnt_greedy_pick) whose `live` mask says which rows emitted, and one masked prediction-network
    # step on the existing embedding / LSTM / GRU kernels (rows that emitted nothing keep h, c and hence lin_dec's d).  Nothing is
    # read by the host inside the frame loop; tokens, lengths and scores of all rows come back in ONE buffer at the end.
    # The state is kept twice (frame t reads copy (t + 1) % 2 and writes copy t % 2: the one-launch LSTM step cannot update h in
    # place), so the unit that repeats is a PAIR of frames; with `graph_steps` that pair is captured once per signature, reads the
    # frame counter from the device and is replayed ceil(T / 2) times (a frame beyond an utterance's length is never live).
    graph_steps = False               # opt-in, as on BeamSearch: the second call of a signature captures, later ones replay
    graph_frame_bucket = 32
    graph_max_signatures = 16
    greedy_max_rows = 64              # rows per frame loop (eamd_rnnt_greedy_*, eamd_lstm_step_fwd); larger batches go in chunks

    def _greedy_batched_ok(self):
        from .transducer.rnn_decoder import DecoderRNNT
        dec = self.decoder
        return type(dec) is DecoderRNNT and not (dec.training and dec.dropout > 0) and ops.get_precision() == "fp32"

    @ops.inference_call
    def greedy_batch(self, hs_pad, hlens=None):
        """hs_pad (B, T, D_enc) encoder states on the device, hlens (list / tensor / None = every row runs all T frames)
        -> [Hypothesis(score, yseq)] * B, yseq[0] == blank: what __call__ returns per utterance with beam_size <= 1.
        DecoderRNNT (lstm / gru): the batched frame loop above, one blocking host read per call.  Other prediction networks:
        a loop over the per-utterance search."""
        if not self._greedy_batched_ok():
            return self._fallback("_greedy", hs_pad, hlens)
        B, T = hs_pad.shape[:2]
        with torch.no_grad():
            _frames, hl = self._lengths(hlens, B, T, hs_pad.device)
            res = self._chunks(hs_pad, self.greedy_max_rows, lambda enc, b0, b1: self._greedy_rows(enc[b0:b1], hl[b0:b1]))
        return [Hypothesis(score=float(r["score"][i]), yseq=r["yseq"][i, :r["ylen"][i]].tolist())
                for r in res for i in range(len(r["ylen"]))]

    @staticmethod
    def _greedy_layout(n, ycap):
        return [("yseq", (n, ycap), np.int32), ("ylen", (n,), np.int32), ("score", (n,), np.float32)]

    def _greedy_ws(self, n, Tcap, dev):
        """the buffers of one frame loop on n rows: the result buffer with its fields as views, both copies of the prediction
        network's state, the step's intermediates and the device frame counter"""
        dec = self.decoder
        J = dec.joint_dim
        ws = self._pred_ws(n, dev)
        ws.update(Tcap=Tcap, layout=self._greedy_layout(n, Tcap + 1), graph=None, calls=0)
        fields = list(_fields(ws["layout"]))
        ws["res"] = torch.empty(fields[-1][3] + fields[-1][4], device=dev, dtype=torch.int32)
        for name, shape, dt, o, words in fields:
            ws[name] = ws["res"][o:o + words].view(_TORCH[dt]).view(shape)
        ws["enc"] = torch.zeros(n, Tcap, J, device=dev, dtype=torch.float32)
        ws["hl"] = torch.empty(n, device=dev, dtype=torch.int32)
        ws["t"] = torch.zeros(1, device=dev, dtype=torch.int32)
        ws["part"] = ops.rnnt_greedy_part(n, dec.odim, dev)
        ws["d"] = torch.empty(n, J, device=dev, dtype=torch.float32)
        return ws

    @staticmethod
    def _stack_step(embed, cells, typ, H, ws, src, dst, live):
        """an embedding + LSTMCell / GRUCell stack (the prediction network's, the RNN LM's) on ws.tok from state copy `src` into
        copy `dst` (live: uint8 [n] or None = every row; a masked row keeps h / c) -> the top layer's new h"""
        from .. import rnn_functional as R_
        n = ws["n"]
        x = ops.embed_pe(ws["tok"], embed, None, 1, 1.0)
        for l, cell in enumerate(cells):
            hp, hn, gx = ws["h"][src][l], ws["h"][dst][l], ws["gx"][l]
            ops.linear_into(x, cell.weight_ih, cell.bias_ih, gx)
            if typ == "lstm":
                cp, cn, gates = ws["c"][src][l], ws["c"][dst][l], ws["gates"][l]
                if ops.lstm_step_ok(n, H):
                    ops.lstm_step_fwd(gx, cell.weight_hh, cell.bias_hh, hp, cp, live, hn, cn, None, gates)
                else:
                    R_._rec_gemm(hp, cell.weight_hh, gates, n, 4 * H, H, H, H, 4 * H, bias=cell.bias_hh, R=gx, ldr=4 * H)
                    ops.lstm_cell_fwd(gates, cp, hp, live, hn, cn, None, gates)
            else:
                gh = ws["gh"][l]
                R_._rec_gemm(hp, cell.weight_hh, gh, n, 3 * H, H, H, H, 3 * H, bias=cell.bias_hh)
                ops.gru_cell_fwd(gx, gh, hp, live, hn, None, ws["gates"][l])
            x = hn
        return x

    def _pred_step(self, ws, src, dst, live):
        """prediction network on ws.tok from state copy `src` into copy `dst` (live: uint8 [n] or None = every row), then lin_dec"""
        dec = self.decoder
        x = self._stack_step(dec.embed.weight, dec.decoder, dec.dtype, dec.dunits, ws, src, dst, live)
        ops.linear_into(x, dec.joint_network.lin_dec.weight, None, ws["d"])

    # ---- RNN LM shallow fusion in the alsd / tsd device loops ------------------------------------------------------------
    # In alsd and tsd the LM advances exactly when the prediction network does: a hypothesis that appends a token steps both, one
    # that appends nothing keeps both states.  ClassifierWithState(RNNLM) is an embedding + LSTMCell / GRUCell stack + Linear, so
    # its state rides in the same copies / blocks as the prediction network's (_lm_ws), moves in the same eamd_gather_rows launch by
    # the same parent rows and steps through the same masked kernels (_stack_step).  Its log-probabilities are computed for all R
    # rows of a pass from the top layer's h (lo + eamd_log_softmax_rows; row r belongs to slot r, so lm_row is an iota and nothing
    # [R, V]-sized is ever gathered); eamd_transducer_expand_rows picks the chosen tokens' terms into its record and the *_step_lm
    # kernels add them by the reference's float32 arithmetic (csrc/rnnt_search.h).
    def _lm_batched_ok(self):
        """does the device loop take self.lm?  Asked for (lm_batched), ClassifierWithState(RNNLM) itself (lstm / gru), fp32
        parameters on the prediction network's device, no dropout at work, a finite weight"""
        from .lm import ClassifierWithState, RNNLM
        lm = self.lm
        if not self.lm_batched:
            return False
        if type(lm) is not ClassifierWithState or type(lm.predictor) is not RNNLM:
            return False
        net = lm.predictor
        dev = self.decoder.embed.weight.device
        try:
            finite = math.isfinite(float(self.lm_weight))
        except (TypeError, ValueError):
            return False
        return (finite and net.typ in ("lstm", "gru")
                and all(q.dtype == torch.float32 and q.device == dev for q in net.parameters())
                and not (net.training and any(d.p > 0 for d in net.dropout)))

    def _lm_stack_step(self, ws, src, dst, live):
        """the LM's cell stack on ws.tok from state copy `src` into copy `dst`, masked by `live`"""
        net = self.lm.predictor
        self._stack_step(net.embed.weight, net.rnn, net.typ, net.n_units, ws, src, dst, live)

    def _lm_rows(self, ws, h_top):
        """the LM log-probabilities of all rows from the top layer's h -> ws["logp"] [R, V]"""
        net = self.lm.predictor
        ops.linear_into(h_top, net.lo.weight, net.lo.bias, ws["z"])
        return ops.log_softmax_rows(ws["z"], out=ws["logp"])

    def _nbest_lm(self, hyps):
        """_nbest for scores carried by the float32 rule: a hypothesis with labels divides score / len in float32"""
        if not self.score_norm:
            return self._nbest(hyps)
        return sorted(hyps, key=lambda x: x.score / len(x.yseq) if len(x.yseq) <= 1
                      else float(np.float32(x.score) / np.float32(len(x.yseq))), reverse=True)

    def _frame(self, ws, parity, t, t_dev):
        """one frame: joint + argmax, bookkeeping, masked prediction step (state copy 1 - parity -> copy parity)"""
        jn = self.decoder.joint_network
        ops.rnnt_greedy_joint(ws["enc"], ws["d"], jn.lin_out.weight, jn.lin_out.bias, ws["part"], jn.act_id, t, t_dev)
        ops.rnnt_greedy_pick(ws["part"], ws["hl"], ws["yseq"], ws["ylen"], ws["score"], ws["tok"], ws["live"], ws["Tcap"],
                             self.vocab_size, self.blank, t, t_dev)
        self._pred_step(ws, 1 - parity, parity, ws["live"])

    def _greedy_rows(self, enc, hl):
        """the frame loop on n <= greedy_max_rows rows: enc (n, T, J) projected encoder states, hl (n,) int32 on the device
        -> (result buffer, its layout), not yet read"""
        from .. import graphs
        n, T, _J = enc.shape
        dev = enc.device
        ws = None
        if self.graph_steps:
            fb = self.graph_frame_bucket
            Tcap = (T + fb - 1) // fb * fb
            dec = self.decoder
            sig = (n, Tcap, dev.index, dec.embed.weight.data_ptr(), dec.joint_network.lin_out.weight.data_ptr())
            if not hasattr(self, "_greedy_graphs"):
                self._greedy_graphs = {}
            ws = self._greedy_graphs.pop(sig, None)
            while len(self._greedy_graphs) >= self.graph_max_signatures:
                self._greedy_graphs.pop(next(iter(self._greedy_graphs)))
            if ws is None:
                ws = self._greedy_ws(n, Tcap, dev)
            self._greedy_graphs[sig] = ws                      # most recently used last
        else:
            ws = self._greedy_ws(n, T, dev)
        ws["calls"] += 1
        ws["enc"][:, :T].copy_(enc)
        ws["hl"].copy_(hl)
        ws["yseq"].fill_(self.blank)
        ws["ylen"].fill_(1)
        ws["score"].zero_()
        ws["tok"].fill_(self.blank)
        for l in range(self.decoder.dlayers):
            ws["h"][0][l].zero_()
            ws["c"][0][l].zero_()
        self._pred_step(ws, 0, 1, None)                        # the initial step on blank from the zero state
        if self.graph_steps and ws["calls"] >= 2:
            try:
                if ws["graph"] is None:
                    torch.cuda.synchronize()
                    g = graphs.new_graph()
                    with torch.cuda.graph(g):
                        self._frame(ws, 0, 0, ws["t"])
                        self._frame(ws, 1, 0, ws["t"])
                    graphs.audit(g, "greedy transducer frame graph")
                    ws["graph"] = g
                ws["t"].zero_()
                for _ in range((T + 1) // 2):
                    ws["graph"].replay()
                return ws["res"].clone(), ws["layout"]
            except Exception as e:  # noqa: BLE001 - a step that cannot be captured: eager frame loops from now on
                import logging
                logging.getLogger(__name__).warning("greedy transducer frame graph disabled: %s", str(e)[:200])
                torch.cuda.synchronize()
                self.graph_steps = False
                self._greedy_graphs = {}
                return self._greedy_rows(enc, hl)
        for t in range(T):
            self._frame(ws, t & 1, t, None)
        return (ws["res"].clone() if self.graph_steps else ws["res"]), ws["layout"]

    # ---- default beam search ----------------------------------------------------------------------------------------
    def _default(self, h):
        self._start(h)
        enc = self.decoder.joint_network.project_enc(h)
        beam = min(self.beam_size, self.vocab_size)
        beam_k = min(beam, self.vocab_size - 1)
        carried = [(0.0, 0)]                    # set B of the previous frame: (score, node)
        for t in range(enc.shape[0]):
            frontier = carried                  # set A
            carried = []
            scored = {}                         # node -> (blank logp, [(logp, token)] best non-blank extensions) at frame t

            def score_pending(first):
                """joint rows for `first` and every other node of the frontier that has none at this frame"""
                nodes = [first] + [n for _s, n in frontier if n not in scored and n != first]
                nodes = list(dict.fromkeys(nodes))
                self._ensure_pred(nodes)
                logp = self._rows(enc[t].unsqueeze(0).expand(len(nodes), -1), nodes)
                top_v, top_i = logp[:, 1:].topk(beam_k, dim=-1)
                host = torch.cat([logp[:, :1], top_v, (top_i + 1).float()], dim=1).tolist()
                for n, row in zip(nodes, host):
                    scored[n] = (row[0], list(zip(row[1:1 + beam_k], (int(v) for v in row[1 + beam_k:]))))

            while True:
                j = max(range(len(frontier)), key=lambda i: frontier[i][0])          # first maximum, as max() over a list
                s_best, n_best = frontier.pop(j)
                if n_best not in scored:
                    score_pending(n_best)
                blank_lp, ext = scored[n_best]
                lm_lp = self._lm_step(n_best) if self.lm else None
                for lp, tok in ext:
                    s = s_best + lp
                    if lm_lp is not None:
                        s += self.lm_weight * lm_lp[tok]
                    frontier.append((s, self._tree.child(n_best, tok)))
                carried.append((s_best + blank_lp, n_best))
                bound = max(s for s, _n in frontier)
                ahead = sorted((c for c in carried if c[0] > bound), key=lambda c: c[0])
                if len(ahead) >= beam:
                    carried = ahead
                    break
        hyps = [Hypothesis(score=s, yseq=self._tree.labels(n)) for s, n in carried]
        if self.score_norm:
            return sorted(hyps, key=lambda x: x.score / len(x.yseq), reverse=True)
        return sorted(hyps, key=lambda x: x.score, reverse=True)

    # ---- batched default ------------------------------------------------------------------------------------------------
    # The default search pops the best entry of A until W entries of B beat everything left in A: how many pops a frame takes
    # depends on the data, so a batch cannot advance frame by frame.  It advances POP by pop: every utterance finishes one pop per
    # step and keeps its own frame counter on the device; a finished one is masked.  Three facts carry the design.  (1) B gains one
    # entry per pop and a frame needs W of them ahead of A, so an utterance of T_b frames takes at least W T_b pops: the first
    # W max(T_b) steps are enqueued without asking.  (2) Without an LM a child scores at most its parent, so max(A) never rises
    # within a frame and an entry with P or more entries ahead of it (score descending, then insertion order) cannot be popped
    # within the next P pops: with at most P = default_max_pops pops per frame A needs P entries, kept sorted, and the reference's
    # first maximum is entry 0.  (3) only popped entries reach B, so every prediction-network state the next frame reads was
    # written by a pop of this frame: the state pool has 2 P rows per utterance, one region per frame parity, and pop i of a frame
    # writes row i of its region (a pop of a carried entry copies its state forward: its `live` is 0, the masked cells pass h / c
    # through, and lin_dec is recomputed, so d is stored nowhere).  Labels are not kept on the device: every pop appends one
    # (parent record, token) pair to the utterance's log and the host rebuilds the sequences after the result copy.
    # One step on n rows (not n W): eamd_gather_rows (h / c by the parent's pool row, the encoder row by b T + t_b), the masked
    # _pred_step, eamd_scatter_rows (the new h / c into the pop's pool row), joint_rows_d, eamd_transducer_expand_rows with its
    # record left on the device, eamd_rnnt_default_step (csrc/rnnt_default.hip: finishes the pop, ends the frame when W entries of B
    # are ahead, selects the next pop).  The host loop only enqueues; after the first W max(T_b) steps, and after every further
    # default_chunk_steps, it reads the done / overflow flags in one small copy, and stops when every utterance has stopped or
    # default_step_budget W max(T_b) steps are spent.  Then ONE result copy.  An utterance whose frame wanted a (P + 1)-th pop, or
    # that the budget cut off, has overflowed and is searched again by the per-utterance search: the answer is always the exact one.
    default_max_pops = 256            # P: pops per frame before an utterance overflows (the kernel takes W <= P <= 256).  A guess
    default_chunk_steps = 64          # steps between two reads of the flags after the first W max(T_b).  A guess
    default_step_budget = 8           # steps at most, in units of W max(T_b).  A guess
    default_max_rows = 64             # utterances per step loop; larger batches go in chunks.  A guess, not a measurement

    def _default_batched_ok(self):
        return self._greedy_batched_ok() and self.lm is None and self.beam_size <= 16

    @ops.inference_call
    def default_batch(self, hs_pad, hlens=None):
        """hs_pad (B, T, D_enc) encoder states on the device, hlens (list / tensor / None = every row runs all T frames)
        -> B n-best lists, each what __call__ returns for hs_pad[b, :hlens[b]] with search_type="default": the last frame's B sorted
        by score / len(yseq) (score with score_norm=False); [Hypothesis(0.0, [blank])] for a row without frames.
        DecoderRNNT (lstm / gru) without an LM, fp32, beam_size <= 16: the batched step loop above.  `passes` is the number of steps
        enqueued, `host_reads` the blocking reads (flags + the one result copy), `overflowed` the utterances that were searched
        again per utterance, `pops` per utterance (pops, frames, most pops of one frame) as the device counted them.
        Anything else: a loop over the per-utterance search."""
        self.passes = self.host_reads = 0
        self.overflowed, self.pops = [], []
        if not self._default_batched_ok():
            return self._fallback("_default", hs_pad, hlens)
        B, T = hs_pad.shape[:2]
        W = min(self.beam_size, self.vocab_size)
        P = min(max(int(self.default_max_pops), W), 256)
        with torch.no_grad():
            frames, hl = self._lengths(hlens, B, T, hs_pad.device)    # a device tensor: the padded T bounds the first chunk
            res = self._chunks(hs_pad, max(1, int(self.default_max_rows)), lambda enc, b0, b1: self._default_rows(
                enc[b0:b1], hl[b0:b1].contiguous(), W, P, max(frames[b0:b1])))
            self.host_reads += 1                                       # the call's one result copy
        out = []
        for r in res:
            score, b_log, ctr, flags, lens, log = (r[name] for name in ("b_score", "b_log", "ctr", "flags", "hl", "log"))
            for b in range(len(lens)):
                g = len(out)
                self.pops.append((int(ctr[b, 4]) if lens[b] else 0, int(lens[b]), int(ctr[b, 7])))
                if flags[1, b] or not flags[0, b]:             # overflowed, or still running when the budget was spent
                    self.overflowed.append(g)
                    out.append(self._one("_default", hs_pad[g, :int(lens[b])]))
                    continue
                labels = {0: [self.blank]}
                hyps = []
                for j in range(int(ctr[b, 3])):
                    node, todo = int(b_log[b, j]), []
                    while node not in labels:
                        todo.append(node)
                        node = int(log[b, node, 0])
                    for m in reversed(todo):
                        par, tk = int(log[b, m, 0]), int(log[b, m, 1])
                        labels[m] = labels[par] + [tk] if tk else labels[par]
                    hyps.append(Hypothesis(score=float(score[b, j]), yseq=list(labels[int(b_log[b, j])])))
                out.append(self._nbest(hyps))
        return out

    @staticmethod
    def _default_layout(n, P, used):
        """B's scores and records, the counters, the flags, the lengths and the `used` filled records per utterance of the log"""
        return [("b_score", (n, P), np.float64), ("b_log", (n, P), np.int32), ("ctr", (n, 8), np.int32), ("flags", (2, n), np.int32),
                ("hl", (n,), np.int32), ("log", (n, used, 2), np.int32)]

    def _default_ws(self, n, P, log_cap, dev):
        """the buffers of one step loop on n utterances: A, B, the pending pop, counters, flags and the label log, what
        eamd_rnnt_default_step leaves for the rest of the step, the state pool of 2 P rows per utterance, and the step's intermediates"""
        dec = self.decoder
        H, L, J = dec.dunits, dec.dlayers, dec.joint_dim
        f = dict(device=dev, dtype=torch.float32)
        i32 = dict(device=dev, dtype=torch.int32)
        ws = self._pred_ws(n, dev)                             # `live` starts at 0: the first step's pop is a carried entry
        ws["A"] = (torch.zeros(n, P, device=dev, dtype=torch.float64),) + tuple(torch.zeros(n, P, **i32) for _ in range(4))
        ws["B"] = (torch.zeros(n, P, device=dev, dtype=torch.float64),) + tuple(torch.zeros(n, P, **i32) for _ in range(2))
        ws["cur"] = torch.zeros(n, device=dev, dtype=torch.float64)
        ws["ctr"] = torch.zeros(n, 8, **i32)
        ws["log"] = torch.empty(n, log_cap, 2, **i32)          # sized to the step budget: only record 0 is filled
        ws["flags"] = torch.zeros(2, n, **i32)
        ws["par"] = torch.empty(n, **i32)
        ws["dst"] = torch.empty(n, **i32)
        ws["frame"] = torch.empty(n, **i32)
        ws["alive"] = torch.empty(n, device=dev, dtype=torch.uint8)
        ws["encr"] = torch.empty(n, J, **f)
        ws["d"] = torch.empty(n, J, **f)
        ws["pool_h"] = [torch.zeros(n * 2 * P, H, **f) for _ in range(L)]
        ws["pool_c"] = [torch.zeros(n * 2 * P, H, **f) for _ in range(L)]
        return ws

    def _default_rows(self, enc, hl, W, P, frames):
        """the step loop on n utterances: enc (n, T, J) projected encoder states, hl (n,) int32 on the device, `frames` = the most
        frames an utterance has -> (result buffer, its layout (_default_layout)); the flags are read here, the buffer is not"""
        n, T, J = enc.shape
        dev = enc.device
        dec, jn, V = self.decoder, self.decoder.joint_network, self.vocab_size
        k = min(W, V - 1)
        first = W * frames
        budget = first * max(1, int(self.default_step_budget))
        ws = self._default_ws(n, P, budget + 1, dev)
        enc_rows = enc.reshape(n * T, J)
        lstm = dec.dtype == "lstm"
        layers = range(dec.dlayers)
        # before frame 0: A = [(0.0, [blank])], and that entry is the first pop: record 0, its state in row 0 of the odd region
        rows = torch.arange(n, device=dev, dtype=torch.int32)
        run = (hl > 0)
        ws["flags"][0].copy_(~run)
        ws["ctr"][:, 1].copy_(run)                             # pops of frame 0: the pending one
        ws["ctr"][:, 3].copy_(~run)                            # an utterance without frames: B = [(0.0, [blank])]
        ws["ctr"][:, 4].fill_(1)
        ws["log"][:, 0, 0].fill_(-1)
        ws["log"][:, 0, 1].zero_()
        ws["par"].copy_(rows * (2 * P) + P)
        ws["dst"].copy_(rows * (2 * P))
        ws["frame"].copy_(rows * T)
        ws["alive"].copy_(run)
        self._pred_step(ws, 0, 1, None)                        # the initial step on blank from the zero state
        jobs = [(ws["pool_h"][l], ws["h"][1][l], ws["par"], None) for l in layers]
        if lstm:
            jobs += [(ws["pool_c"][l], ws["c"][1][l], ws["par"], None) for l in layers]
        ops.scatter_rows(jobs)
        gather = [(ws["encr"], enc_rows, ws["frame"])] + [(ws["h"][0][l], ws["pool_h"][l], ws["par"]) for l in layers]
        scatter = [(ws["pool_h"][l], ws["h"][1][l], ws["dst"], ws["alive"]) for l in layers]
        if lstm:
            gather += [(ws["c"][0][l], ws["pool_c"][l], ws["par"]) for l in layers]
            scatter += [(ws["pool_c"][l], ws["c"][1][l], ws["dst"], ws["alive"]) for l in layers]

        def step():
            ops.gather_rows(gather)
            self._pred_step(ws, 0, 1, ws["live"])
            ops.scatter_rows(scatter)
            rec = ops.transducer_expand_rows_dev(jn.joint_rows_d(ws["encr"], ws["d"]), k)
            ops.rnnt_default_step(rec, hl, ws["A"], ws["B"], ws["cur"], ws["ctr"], ws["log"], ws["flags"], ws["par"], ws["tok"],
                                  ws["dst"], ws["live"], ws["frame"], ws["alive"], W, V, T)

        steps = first
        for _ in range(first):
            step()
        while True:
            flags = ws["flags"].cpu().numpy()                  # one small blocking copy
            self.host_reads += 1
            if bool((flags[0] | flags[1]).all()) or steps >= budget:
                break
            more = min(max(1, int(self.default_chunk_steps)), budget - steps)
            for _ in range(more):
                step()
            steps += more
        self.passes += steps
        layout = self._default_layout(n, P, steps + 1)
        return _pack(layout, [ws["B"][0], ws["B"][2], ws["ctr"], ws["flags"], hl, ws["log"][:, :steps + 1]]), layout

    # ---- tsd / alsd / nsc: passes --------------------------------------------------------------------------------------
    def _batch_pred(self, nodes):
        """prediction outputs of `nodes` (one of the reference's batch_score calls: the hypotheses in its order)"""
        if self.batched:
            self._ensure_pred(nodes)
            return
        todo = [n for n in dict.fromkeys(nodes) if n not in self._pred.out]      # first computation wins
        if todo:
            y = self.decoder.batch_step([self._tree.labels(n) for n in todo])
            for i, n in enumerate(todo):
                self._pred.out[n] = y[i]

    def _ensure_lm(self, nodes):
        """LM log-probabilities of the token after each node, all missing nodes in one batch (buff_predict)"""
        pr, tr = self._pred, self._tree
        todo = [n for n in dict.fromkeys(nodes) if n not in pr.lm_dev]
        if 0 in todo:                           # the root: from the LM's zero state, alone (it is only ever first)
            todo.remove(0)
            self._lm_batch([0], None)
        if todo:
            prev = [pr.lm_state[tr.parent[n]] for n in todo]
            self._lm_batch(todo, {key: [torch.stack([p[key][l] for p in prev]) for l in range(len(prev[0][key]))]
                                  for key in prev[0]})

    def _lm_batch(self, todo, state):
        pr = self._pred
        tok = torch.tensor([self._tree.token[n] for n in todo], dtype=torch.long).to(self._init_tensor.device)
        new, logp = self.lm.predict(state, tok)
        for i, n in enumerate(todo):
            pr.lm_state[n] = {key: [layer[i] for layer in new[key]] for key in new}
            pr.lm_dev[n] = (logp, i)

    def _expand(self, enc_rows, nodes, k, pairs=None):
        """one search pass on len(nodes) (encoder row, node) pairs: joint rows + eamd_transducer_expand_rows, ONE blocking
        read -> ops.transducer_expand_rows's (rows, pair log-probabilities)"""
        logits = self.decoder.joint_network.joint_rows(enc_rows, torch.stack([self._pred.out[n] for n in nodes]))
        lm = lm_row = None
        if self.lm is not None:
            self._ensure_lm(nodes)
            mats, lm_row = {}, []
            for n in nodes:
                m, r = self._pred.lm_dev[n]
                base = mats.setdefault(id(m), (m, sum(x.shape[0] for x, _b in mats.values())))[1]
                lm_row.append(base + r)
            lm = next(iter(mats.values()))[0] if len(mats) == 1 else torch.cat([m for m, _b in mats.values()])
        self.passes += 1
        self.host_reads += 1
        return ops.transducer_expand_rows(logits, k, lm=lm, lm_row=lm_row, pairs=pairs)

    def _lm_term(self, lm_lp):
        """lm_weight * beam_lm_scores[i, k] of the reference: a float32 0-d tensor (the score it is added to becomes one)"""
        return self.lm_weight * torch.tensor(lm_lp, dtype=torch.float32)

    def _sort_nbest(self, hyps):
        return self._result(self._nbest(hyps, lambda x: len(self._tree.labels(x.node))))

    def _result(self, hyps):
        return [Hypothesis(score=float(x.score), yseq=self._tree.labels(x.node)) for x in hyps]

    def _start_passes(self, h):
        self._start(h)
        self.passes = self.host_reads = 0
        return self.decoder.joint_network.project_enc(h)

    # ---- time synchronous decoding (reference :239-347) ----------------------------------------------------------------
    def _tsd(self, h):
        enc = self._start_passes(h)
        beam = min(self.beam_size, self.vocab_size)
        k = min(beam, self.vocab_size - 1)
        B = [_Hyp(0.0, 0)]
        for t in range(enc.shape[0]):
            A = []
            C = B
            for _v in range(self.max_sym_exp):          # the reference's `v < max_sym_exp` always holds: every pass expands
                nodes = [c.node for c in C]
                self._batch_pred(nodes)
                rows, _ = self._expand(enc[t].unsqueeze(0).expand(len(C), -1), nodes, k)
                seq_A = [a.node for a in A]
                for c, (blank_lp, _ext, _lm) in zip(C, rows):
                    if c.node not in seq_A:
                        A.append(_Hyp(c.score + blank_lp, c.node))
                    else:
                        a = A[seq_A.index(c.node)]
                        a.score = np.logaddexp(a.score, c.score + blank_lp)
                D = []
                for c, (_b, ext, lm_lp) in zip(C, rows):
                    for j, (lp, tok) in enumerate(ext):
                        s = c.score + lp
                        if lm_lp is not None:
                            s += self._lm_term(lm_lp[j])
                        D.append(_Hyp(s, self._tree.child(c.node, tok)))
                C = sorted(D, key=lambda x: x.score, reverse=True)[:beam]
            B = sorted(A, key=lambda x: x.score, reverse=True)[:beam]
        return self._sort_nbest(B)

    # ---- alignment-length synchronous decoding (reference :349-464) ----------------------------------------------------
    def _alsd(self, h):
        enc = self._start_passes(h)
        beam = min(self.beam_size, self.vocab_size)
        k = min(beam, self.vocab_size - 1)
        T = enc.shape[0]
        u_max = min(self.u_max, T - 1)
        depth = [0]                                     # node -> u = len(yseq) - 1
        B = [_Hyp(0.0, 0)]
        final = []
        for i in range(T + u_max):
            B_, ts = [], []
            for b in B:
                while len(depth) <= b.node:
                    depth.append(depth[self._tree.parent[len(depth)]] + 1)
                t = i - depth[b.node] + 1               # >= 1: frame 0 is never scored (reference)
                if t > T - 1:
                    continue
                B_.append(b)
                ts.append(t)
            if not B_:
                continue
            nodes = [b.node for b in B_]
            self._batch_pred(nodes)
            rows, _ = self._expand(enc[torch.tensor(ts, dtype=torch.long).to(enc.device)], nodes, k)
            A = []
            for b, t, (blank_lp, ext, lm_lp) in zip(B_, ts, rows):
                nb = _Hyp(b.score + blank_lp, b.node)
                A.append(nb)
                if t == T - 1:
                    final.append(nb)
                for j, (lp, tok) in enumerate(ext):
                    s = b.score + lp
                    if lm_lp is not None:
                        s += self._lm_term(lm_lp[j])
                    A.append(_Hyp(s, self._tree.child(b.node, tok)))
            B = sorted(A, key=lambda x: x.score, reverse=True)[:beam]
            seen = []                                   # recombine_hyps (transducer/utils.py:181-203): B itself is kept
            for b in B:
                if b.node in [f.node for f in seen]:
                    f = seen[[f.node for f in seen].index(b.node)]
                    f.score = np.logaddexp(f.score, b.score)
                else:
                    seen.append(b)
        if final:
            return self._sort_nbest(final)
        return self._result(B)

    # ---- batched alsd ---------------------------------------------------------------------------------------------------
    # Every alsd hypothesis consumes one (frame, label prefix) pair per step and the step count is fixed, so the utterances of a batch
    # advance in lock-step as they do in greedy_batch.  Row r = b * W + w is slot w of utterance b (W = min(beam_size, V)).  One step
    # is joint_rows_d on the rows' gathered encoder frames and lin_dec outputs, eamd_transducer_expand_rows with its record left on the
    # device, eamd_rnnt_alsd_step (the A / B / final bookkeeping of _alsd, one workgroup per utterance: it leaves the parent row, the
    # token, the `live` mask and the next encoder row of every slot), ONE eamd_gather_rows launch (encoder rows by frame, h / c of
    # every layer by parent row, from state copy 1 into copy 0) and the masked prediction step of _pred_step from copy 0 back into
    # copy 1.  The host loop only enqueues launches; finals and the last B of all utterances come back in ONE copy, and the n-best
    # sort of the reference happens on the host after it.
    alsd_max_rows = 256               # rows (utterances x W) per step loop; larger batches go in chunks.  A guess, not a measurement

    def _alsd_batched_ok(self):
        return self._greedy_batched_ok() and (self.lm is None or self._lm_batched_ok()) and self.beam_size <= 16

    @ops.inference_call
    def alsd_batch(self, hs_pad, hlens=None):
        """hs_pad (B, T, D_enc) encoder states on the device, hlens (list / tensor / None = every row runs all T frames)
        -> B n-best lists, each what __call__ returns for hs_pad[b, :hlens[b]] with search_type="alsd": the final hypotheses sorted
        by score / len(yseq) (score with score_norm=False), or B in slot order when no hypothesis reached the last frame.
        DecoderRNNT (lstm / gru), fp32, beam_size <= 16, without an LM or - with lm_batched=True - with ClassifierWithState(RNNLM)
        (_lm_batched_ok): the batched step loop above, one blocking host read per call.  With an LM the scores of hypotheses with
        labels hold float32 values, as
        the per-utterance search carries them, and the n-best sort divides in float32.
        Anything else (an LM without lm_batched, nsc / default with an LM, a TransformerLM, an LM with dropout at work): a loop
        over the per-utterance search."""
        if not self._alsd_batched_ok():
            return self._fallback("_alsd", hs_pad, hlens)
        B, T = hs_pad.shape[:2]
        W = min(self.beam_size, self.vocab_size)
        u_max = int(self.u_max)
        with torch.no_grad():
            frames, hl = self._lengths(hlens, B, T, hs_pad.device)    # a device tensor: the padded T bounds every utterance
            steps = [t + min(u_max, t - 1) for t in frames]
            res = self._chunks(hs_pad, max(1, self.alsd_max_rows // W), lambda enc, b0, b1: self._alsd_rows(
                enc[b0:b1], hl[b0:b1], W, u_max, max(steps[b0:b1])))
        nbest = self._nbest if self.lm is None else self._nbest_lm
        out = []
        for r in res:
            for b in range(len(r["nfin"])):
                if r["nfin"][b]:
                    out.append(nbest([Hypothesis(score=float(r["fin_score"][b, j]),
                                                       yseq=r["fin_yseq"][b, j, :r["fin_len"][b, j]].tolist())
                                            for j in range(r["nfin"][b])]))
                else:
                    out.append([Hypothesis(score=float(r["score"][b, m]), yseq=r["yseq"][b, m, :r["ulen"][b, m] + 1].tolist())
                                for m in range(r["nhyp"][b])])
        return out

    @staticmethod
    def _alsd_layout(n, W, T, u_max):
        """the finals (fcap = W (u_max + 2) of them at most, u_max + 2 labels each) and the last B"""
        fw, fcap = u_max + 2, W * (u_max + 2)
        return [("fin_score", (n, fcap), np.float64), ("score", (n, W), np.float64), ("nfin", (n,), np.int32),
                ("fin_len", (n, fcap), np.int32), ("fin_yseq", (n, fcap, fw), np.int32), ("nhyp", (n,), np.int32),
                ("ulen", (n, W), np.int32), ("yseq", (n, W, T + u_max + 1), np.int32)]

    def _alsd_ws(self, n, W, T, u_max, dev):
        """the buffers of one step loop on n utterances x W slots: both parities of the search state, the finals, what
        eamd_rnnt_alsd_step leaves for the rest of the step, both copies of the prediction network's state and the step's intermediates"""
        J = self.decoder.joint_dim
        R = n * W
        fw, fcap = u_max + 2, W * (u_max + 2)
        f = dict(device=dev, dtype=torch.float32)
        i32 = dict(device=dev, dtype=torch.int32)
        ws = self._pred_ws(R, dev)
        ws["st"] = [(torch.zeros(n, W, device=dev, dtype=torch.float64), torch.zeros(n, W, **i32), torch.ones(n, **i32),
                     torch.zeros(n, W, T + u_max + 1, **i32)) for _ in range(2)]
        ws["fin"] = (torch.zeros(n, fcap, device=dev, dtype=torch.float64), torch.zeros(n, fcap, **i32),
                     torch.zeros(n, fcap, fw, **i32), torch.zeros(n, **i32))
        ws["par"] = torch.empty(R, **i32)
        ws["frame"] = torch.empty(R, **i32)
        ws["encr"] = torch.empty(R, J, **f)
        ws["d"] = torch.empty(R, J, **f)
        return ws

    def _alsd_rows(self, enc, hl, W, u_max, steps):
        """the step loop on n utterances: enc (n, T, J) projected encoder states, hl (n,) int32 on the device
        -> (result buffer, its layout (_alsd_layout)), not yet read"""
        n, T, J = enc.shape
        dev = enc.device
        dec, jn, V = self.decoder, self.decoder.joint_network, self.vocab_size
        k = min(W, V - 1)
        ws = self._alsd_ws(n, W, T, u_max, dev)
        enc_rows = enc.reshape(n * T, J)
        self._pred_step(ws, 0, 1, None)                        # the initial step on blank from the zero state, into copy 1
        lm = None
        if self.lm is not None:                                # the LM's step on blank from its zero state, as _ensure_lm's for the root
            lm = self._lm_ws(n * W, ws["tok"], dev)
            self._lm_stack_step(lm, 0, 1, None)
            wf = float(self.lm_weight)
        # step 0 scores slot 0 on frame 1 (t = i - u + 1: frame 0 is never scored), or frame 0 of a one-frame utterance
        first = torch.arange(n, device=dev, dtype=torch.int32) * T + (hl - 1).clamp(0, 1)
        ws["frame"].copy_(first.repeat_interleave(W))
        ops.gather_rows([(ws["encr"], enc_rows, ws["frame"])])
        lstm = dec.dtype == "lstm"
        p = 0
        for i in range(steps):
            logits = jn.joint_rows_d(ws["encr"], ws["d"])
            if lm is None:
                rec = ops.transducer_expand_rows_dev(logits, k)
                ops.rnnt_alsd_step(rec, hl, ws["st"][p], ws["st"][1 - p], ws["fin"], ws["par"], ws["tok"], ws["live"], ws["frame"],
                                   V, T, u_max, i)
            else:
                rec = ops.transducer_expand_rows_lm_dev(logits, k, self._lm_rows(lm, lm["h"][1][-1]), lm["iota"], in_range=True)
                ops.rnnt_alsd_step_lm(rec, hl, ws["st"][p], ws["st"][1 - p], ws["fin"], ws["par"], ws["tok"], ws["live"],
                                      ws["frame"], V, T, u_max, i, wf)
            p = 1 - p
            if i == steps - 1:
                break
            jobs = [(ws["encr"], enc_rows, ws["frame"])]
            for l in range(dec.dlayers):
                jobs.append((ws["h"][0][l], ws["h"][1][l], ws["par"]))
                if lstm:
                    jobs.append((ws["c"][0][l], ws["c"][1][l], ws["par"]))
            if lm is not None:
                for l in range(self.lm.predictor.n_layers):
                    jobs.append((lm["h"][0][l], lm["h"][1][l], ws["par"]))
                    if self.lm.predictor.typ == "lstm":
                        jobs.append((lm["c"][0][l], lm["c"][1][l], ws["par"]))
            ops.gather_rows(jobs)
            self._pred_step(ws, 0, 1, ws["live"])
            if lm is not None:
                self._lm_stack_step(lm, 0, 1, ws["live"])
        score, ulen, nhyp, yseq = ws["st"][p]
        fin_score, fin_len, fin_yseq, nfin = ws["fin"]
        layout = self._alsd_layout(n, W, T, u_max)
        return _pack(layout, [fin_score, score, nfin, fin_len, fin_yseq, nhyp, ulen, yseq]), layout

    # ---- batched tsd ----------------------------------------------------------------------------------------------------
    # tsd takes max_sym_exp = M passes per frame whatever the hypotheses are, so the utterances of a batch advance in lock-step here
    # too.  Hypotheses live in M + 1 blocks of R = n * W rows (W = min(beam_size, V)): block 0 and block M are the two parities of
    # B, block v is the C of pass v; the prediction network's h / c and lin_dec's d are stacked the same way, [(M + 1) R, .], so a
    # block row indexes them directly.  One pass (t, v) is joint_rows_d on the frame's encoder rows and the d rows of C's block,
    # eamd_transducer_expand_rows with its record left on the device, eamd_rnnt_tsd_step (A's update with its merges, and the
    # selection of the next C from D or, after the last pass, of the next B from A: one workgroup per utterance, it leaves the parent
    # block row, the token and the `live` mask of every slot) and ONE eamd_gather_rows launch by parent row: on a pass v < M - 1 h / c
    # into a staging copy, from which the masked _pred_step writes block v + 1; at the frame's end h / c / d into B's other parity,
    # and the next frame's encoder rows.  The host loop only enqueues; the last B of all utterances comes back in ONE copy and is
    # sorted on the host as _sort_nbest sorts it.
    tsd_max_rows = 256                # rows (utterances x W) per pass loop; larger batches go in chunks.  A guess, not a measurement

    def _tsd_batched_ok(self):
        return (self._greedy_batched_ok() and (self.lm is None or self._lm_batched_ok()) and self.beam_size <= 16
                and 1 <= self.max_sym_exp <= 4)

    @ops.inference_call
    def tsd_batch(self, hs_pad, hlens=None):
        """hs_pad (B, T, D_enc) encoder states on the device, hlens (list / tensor / None = every row runs all T frames)
        -> B n-best lists, each what __call__ returns for hs_pad[b, :hlens[b]] with search_type="tsd": the last B sorted by
        score / len(yseq) (score with score_norm=False).
        DecoderRNNT (lstm / gru), fp32, beam_size <= 16, max_sym_exp <= 4, without an LM or - with lm_batched=True - with
        ClassifierWithState(RNNLM) (_lm_batched_ok): the batched pass loop above, one blocking host read per call.  With an LM the
        scores of hypotheses with
        labels hold float32 values, as the per-utterance search carries them, and the n-best sort divides in float32.  The last pass
        of a frame discards D: it computes no LM rows (its record's LM terms come from the buffer of the pass before and are never
        read), but its A update follows the float32 arithmetic like every other.
        Anything else: a loop over the per-utterance search."""
        if not self._tsd_batched_ok():
            return self._fallback("_tsd", hs_pad, hlens)
        B, T = hs_pad.shape[:2]
        W = min(self.beam_size, self.vocab_size)
        M = int(self.max_sym_exp)
        with torch.no_grad():
            frames, hl = self._lengths(hlens, B, T, hs_pad.device)    # a device tensor: all T frames run, finished utterances idle
            res = self._chunks(hs_pad, max(1, self.tsd_max_rows // W), lambda enc, b0, b1: self._tsd_rows(
                enc[b0:b1], hl[b0:b1], W, M, max(frames[b0:b1])))
        return [hyps for r in res for hyps in self._block_nbest(r, self._nbest if self.lm is None else self._nbest_lm)]

    @staticmethod
    def _block_layout(n, W, ycap):
        """tsd / nsc: one hypothesis block, the last B / kept"""
        return [("score", (n, W), np.float64), ("count", (n,), np.int32), ("ulen", (n, W), np.int32), ("yseq", (n, W, ycap), np.int32)]

    def _block_nbest(self, r, nbest=None):
        """the n-best list of every utterance of an unpacked _block_layout"""
        return [(nbest or self._nbest)([Hypothesis(score=float(r["score"][b, m]), yseq=r["yseq"][b, m, :r["ulen"][b, m] + 1].tolist())
                             for m in range(r["count"][b])]) for b in range(len(r["count"]))]

    def _tsd_ws(self, n, W, T, M, dev):
        """the buffers of one pass loop on n utterances x W slots: the M + 1 hypothesis blocks, the frame's A, what eamd_rnnt_tsd_step
        leaves for the rest of the pass, the stacked prediction-network state with its staging copy and the pass's intermediates"""
        J = self.decoder.joint_dim
        R = n * W
        f = dict(device=dev, dtype=torch.float32)
        i32 = dict(device=dev, dtype=torch.int32)
        d = torch.empty((M + 1) * R, J, **f)
        ws = self._block_ws(M + 1, R, [d[j * R:(j + 1) * R] for j in range(M + 1)], dev)
        ws["d"] = d
        ws["st"] = (torch.zeros(M + 1, n, W, device=dev, dtype=torch.float64), torch.zeros(M + 1, n, W, **i32),
                    torch.zeros(M + 1, n, **i32), torch.zeros(M + 1, n, W, 1 + T * (M - 1), **i32))
        ws["st"][2][0].fill_(1)                               # B of frame 0: slot 0 holds [blank] with score 0
        ws["A"] = (torch.zeros(n, W * M, device=dev, dtype=torch.float64), torch.zeros(n, W * M, **i32), torch.zeros(n, **i32))
        ws["par"] = torch.empty(R, **i32)
        ws["encr"] = torch.empty(R, J, **f)
        return ws

    def _tsd_rows(self, enc, hl, W, M, frames):
        """the pass loop on n utterances: enc (n, T, J) projected encoder states, hl (n,) int32 on the device, `frames` frames
        -> (result buffer, its layout (_block_layout of the last B)), not yet read"""
        n, T, J = enc.shape
        dev = enc.device
        dec, jn, V = self.decoder, self.decoder.joint_network, self.vocab_size
        k = min(W, V - 1)
        R = n * W
        ws = self._tsd_ws(n, W, T, M, dev)
        enc_rows = enc.reshape(n * T, J)
        st, blk = ws["st"], ws["blk"]
        self._pred_step(blk[0], 0, 1, None)                    # the initial step on blank from the zero state, into block 0
        lstm = dec.dtype == "lstm"
        lm = None
        if self.lm is not None:                                # the LM's step on blank from its zero state, into block 0
            lm = self._lm_ws(R, ws["tok"], dev, blocks=M + 1)
            lblk = lm["blk"]
            self._lm_stack_step(lblk[0], 0, 1, None)
            wf = float(self.lm_weight)
            lm_layers = range(self.lm.predictor.n_layers)
            lm_lstm = self.lm.predictor.typ == "lstm"
        p = 0
        if frames:
            ft = self._frame_rows(hl, T, W, frames)
            ops.gather_rows([(ws["encr"], enc_rows, ft[0])])
        for t in range(frames):
            for v in range(M):
                cin = (M if p else 0) if v == 0 else v
                cout = v + 1 if v < M - 1 else (0 if p else M)
                logits = jn.joint_rows_d(ws["encr"], blk[cin]["d"])
                if lm is None:
                    rec = ops.transducer_expand_rows_dev(logits, k)
                    ops.rnnt_tsd_step(rec, hl, st, ws["A"], ws["par"], ws["tok"], ws["live"], V, T, M, t, v, p)
                else:
                    # the last pass builds no D: its LM terms are never read, so the buffer of the pass before stands in for them
                    logp = self._lm_rows(lm, lblk[cin]["h"][1][-1]) if v < M - 1 else lm["logp"]
                    rec = ops.transducer_expand_rows_lm_dev(logits, k, logp, lm["iota"], in_range=True)
                    ops.rnnt_tsd_step_lm(rec, hl, st, ws["A"], ws["par"], ws["tok"], ws["live"], V, T, M, t, v, p, wf)
                if v < M - 1:
                    jobs = [(blk[cout]["h"][0][l], ws["h"][l], ws["par"]) for l in range(dec.dlayers)]
                    if lstm:
                        jobs += [(blk[cout]["c"][0][l], ws["c"][l], ws["par"]) for l in range(dec.dlayers)]
                    if lm is not None:
                        jobs += [(lblk[cout]["h"][0][l], lm["h"][l], ws["par"]) for l in lm_layers]
                        if lm_lstm:
                            jobs += [(lblk[cout]["c"][0][l], lm["c"][l], ws["par"]) for l in lm_layers]
                elif t == frames - 1:
                    break                                      # the last B's prediction state is never read
                else:
                    jobs = [(blk[cout]["h"][1][l], ws["h"][l], ws["par"]) for l in range(dec.dlayers)]
                    if lstm:
                        jobs += [(blk[cout]["c"][1][l], ws["c"][l], ws["par"]) for l in range(dec.dlayers)]
                    jobs += [(blk[cout]["d"], ws["d"], ws["par"]), (ws["encr"], enc_rows, ft[t + 1])]
                    if lm is not None:
                        jobs += [(lblk[cout]["h"][1][l], lm["h"][l], ws["par"]) for l in lm_layers]
                        if lm_lstm:
                            jobs += [(lblk[cout]["c"][1][l], lm["c"][l], ws["par"]) for l in lm_layers]
                ops.gather_rows(jobs)
                if v < M - 1:
                    self._pred_step(blk[cout], 0, 1, ws["live"])
                    if lm is not None:
                        self._lm_stack_step(lblk[cout], 0, 1, ws["live"])
            p = 1 - p
        last = M if p else 0
        layout = self._block_layout(n, W, 1 + T * (M - 1))
        return _pack(layout, [st[0][last], st[2][last], st[1][last], st[3][last]]), layout

    # ---- N-step constrained beam search (reference :466-663) -----------------------------------------------------------
    def _nsc(self, h):
        enc = self._start_passes(h)
        beam = min(self.beam_size, self.vocab_size)
        k = min(beam, self.vocab_size - 1)
        tr = self._tree
        self._batch_pred([0])
        if self.lm is not None:
            self._ensure_lm([0])
        labels = {}

        def seq(node):
            if node not in labels:
                labels[node] = tr.labels(node)
            return labels[node]

        kept = [_Hyp(0.0, 0)]
        for t in range(enc.shape[0]):
            hyps = sorted(kept, key=lambda x: len(seq(x.node)), reverse=True)
            # prefix rescoring: hyps[j] gains logaddexp(., hyps[i].score + the log-probabilities of the rest of its labels) for
            # every shorter hyps[i] that is a prefix of it within prefix_alpha labels.  Scores read are those of i > j, not yet
            # updated, so every needed term comes from the pass below: rows = the prefix nodes, pairs = (row, next label)
            todo = []
            for j in range(len(hyps) - 1):
                yj = seq(hyps[j].node)
                for i in range(j + 1, len(hyps)):
                    yi = seq(hyps[i].node)
                    if len(yi) < len(yj) and yj[:len(yi)] == yi and len(yj) - len(yi) <= self.prefix_alpha:
                        todo.append((j, i))
            nodes = [x.node for x in hyps]
            pairs, terms = [], []
            if todo:
                row_of = {n: r for r, n in reversed(list(enumerate(nodes)))}
                for j, i in todo:
                    yj = seq(hyps[j].node)
                    path, n = [], hyps[j].node          # path[m] = node of yj[:m + 1]
                    while n >= 0:
                        path.append(n)
                        n = tr.parent[n]
                    path.reverse()
                    idx = []
                    for m in range(len(seq(hyps[i].node)) - 1, len(yj) - 1):
                        if path[m] not in row_of:
                            row_of[path[m]] = len(nodes)
                            nodes.append(path[m])
                        idx.append(len(pairs))
                        pairs.append((row_of[path[m]], yj[m + 1]))
                    terms.append(idx)
            self._batch_pred(nodes)
            rows, pair_lp = self._expand(enc[t].unsqueeze(0).expand(len(nodes), -1), nodes, k, pairs)
            for (j, i), idx in zip(todo, terms):
                curr = hyps[i].score + pair_lp[idx[0]]
                for q in idx[1:]:
                    curr += pair_lp[q]
                hyps[j].score = np.logaddexp(hyps[j].score, curr)
            S = []
            for n in range(self.nstep):
                if n > 0:
                    if not hyps:
                        break
                    rows, _ = self._expand(enc[t].unsqueeze(0).expand(len(hyps), -1), [x.node for x in hyps], k)
                V = []
                for x, (blank_lp, ext, lm_lp) in zip(hyps, rows):
                    for j, (lp, tok) in enumerate(ext):
                        s = x.score + lp
                        if lm_lp is not None:
                            s += self.lm_weight * lm_lp[j]
                        V.append(_Hyp(s, tr.child(x.node, tok)))
                    nb = _Hyp(x.score + blank_lp, x.node)
                    S.append(nb)
                    V.append(nb)
                V = sorted(V, key=lambda x: x.score, reverse=True)
                in_hyps = {x.node for x in hyps}
                V = [v for v in V if v.node not in in_hyps][:beam]          # substract (transducer/utils.py:75-93)
                self._batch_pred([v.node for v in V])
                if self.lm is not None:
                    self._ensure_lm([v.node for v in V])
                if n < self.nstep - 1:
                    hyps = V[:]
                elif self.nstep != 1 and V:
                    last, _ = self._expand(enc[t].unsqueeze(0).expand(len(V), -1), [v.node for v in V], 1)
                    for v, r in zip(V, last):
                        v.score += r[0]
            kept = sorted(S + V, key=lambda x: x.score, reverse=True)[:beam]
        return self._sort_nbest(kept)

    # ---- batched nsc ----------------------------------------------------------------------------------------------------
    # nsc takes nstep = N expansions per frame (and, when N > 1, one more pass for the blank term of the last V) whatever the
    # hypotheses are, so the utterances of a batch advance in lock-step here too.  Hypotheses live in N + 2 blocks of R = n * W rows
    # (W = min(beam_size, V)): block 0 and block N + 1 are the two parities of `kept`, block v is the V of n-step v - 1; the
    # prediction network's h / c are stacked the same way, [(N + 2) R, .], and lin_dec's d with the history levels of the prefix
    # rescoring as [N + 2][1 + prefix_alpha][R]: level a of a row is d of its labels without the last a.  One call (t, v) is
    # joint_rows_d on the frame's encoder rows and the d rows of hyps' block - at v == 0 on all (1 + prefix_alpha) R rows of kept's
    # block, so that the same eamd_transducer_expand_rows launch leaves the frame's pair terms by the device-side pair list the
    # previous frame's last call wrote -, eamd_rnnt_nsc_step (prefix rescoring, S, substract and the selection of V or of the next
    # kept: one workgroup per utterance, it leaves the parent block row, the token, the `live` mask and the history rows of every
    # slot) and eamd_gather_rows by those rows: h / c into a staging copy, from which the masked _pred_step writes the next block,
    # and the history levels; at the end of a frame with N > 1 h / c / d / history into kept's other parity; at every frame's end the
    # next frame's encoder rows.  The host loop only enqueues; the last kept of all utterances comes back in ONE copy and is sorted on
    # the host as _sort_nbest sorts it.
    nsc_max_rows = 256                # rows (utterances x W) per frame loop; larger batches go in chunks.  A guess, not a measurement

    def _nsc_batched_ok(self):
        return (self._greedy_batched_ok() and self.lm is None and self.beam_size <= 16 and 1 <= self.nstep <= 4
                and 0 <= self.prefix_alpha <= 3)

    @ops.inference_call
    def nsc_batch(self, hs_pad, hlens=None):
        """hs_pad (B, T, D_enc) encoder states on the device, hlens (list / tensor / None = every row runs all T frames)
        -> B n-best lists, each what __call__ returns for hs_pad[b, :hlens[b]] with search_type="nsc": the last kept sorted by
        score / len(yseq) (score with score_norm=False).
        DecoderRNNT (lstm / gru) without an LM, fp32, beam_size <= 16, nstep <= 4, prefix_alpha <= 3: the batched frame loop above,
        one blocking host read per call.  Anything else: a loop over the per-utterance search."""
        if not self._nsc_batched_ok():
            return self._fallback("_nsc", hs_pad, hlens)
        B, T = hs_pad.shape[:2]
        W = min(self.beam_size, self.vocab_size)
        N, alpha = int(self.nstep), int(self.prefix_alpha)
        with torch.no_grad():
            frames, hl = self._lengths(hlens, B, T, hs_pad.device)    # a device tensor: all T frames run, finished utterances idle
            res = self._chunks(hs_pad, max(1, self.nsc_max_rows // W), lambda enc, b0, b1: self._nsc_rows(
                enc[b0:b1], hl[b0:b1], W, N, alpha, max(frames[b0:b1])))
        return [hyps for r in res for hyps in self._block_nbest(r)]

    def _nsc_ws(self, n, W, T, N, alpha, dev):
        """the buffers of one frame loop on n utterances x W slots: the N + 2 hypothesis blocks, the frame's S, what eamd_rnnt_nsc_step
        leaves for the rest of the call, the pair list and its log-probabilities, the stacked prediction-network state with its
        staging copy, the stacked d / history rows and the call's intermediates"""
        J = self.decoder.joint_dim
        R, LV = n * W, 1 + alpha
        f = dict(device=dev, dtype=torch.float32)
        i32 = dict(device=dev, dtype=torch.int32)
        hs = torch.zeros(N + 2, LV, R, J, **f)                # level 0: d; level a: d of the labels without the last a
        ws = self._block_ws(N + 2, R, [hs[j, 0] for j in range(N + 2)], dev)
        ws["hs"] = hs
        ws["st"] = (torch.zeros(N + 2, n, W, device=dev, dtype=torch.float64), torch.zeros(N + 2, n, W, **i32),
                    torch.zeros(N + 2, n, **i32), torch.zeros(N + 2, n, W, 1 + T * N, **i32))
        ws["st"][2][0].fill_(1)                               # kept of frame 0: slot 0 holds [blank] with score 0
        ws["S"] = (torch.zeros(n, W * N, device=dev, dtype=torch.float64), torch.zeros(n, W * N, **i32), torch.zeros(n, **i32))
        ws["par"] = torch.empty(R, **i32)
        ws["hidx"] = torch.zeros(LV, R, **i32)
        ws["pairs"] = torch.zeros(max(1, R * alpha), 2, **i32)
        ws["pairs"][:, 0].fill_(-1)                           # frame 0: [blank] has no prefix
        ws["pair_lp"] = torch.zeros(max(1, R * alpha), **f)
        ws["encr"] = torch.empty(LV * R, J, **f)
        return ws

    def _nsc_rows(self, enc, hl, W, N, alpha, frames):
        """the frame loop on n utterances: enc (n, T, J) projected encoder states, hl (n,) int32 on the device, `frames` frames
        -> (result buffer, its layout (_block_layout of the last kept)), not yet read"""
        n, T, J = enc.shape
        dev = enc.device
        dec, jn, V = self.decoder, self.decoder.joint_network, self.vocab_size
        k = min(W, V - 1)
        R, LV = n * W, 1 + alpha
        ws = self._nsc_ws(n, W, T, N, alpha, dev)
        enc_rows = enc.reshape(n * T, J)
        st, blk, hs = ws["st"], ws["blk"], ws["hs"]
        hs_rows = hs.view((N + 2) * LV * R, J)
        self._pred_step(blk[0], 0, 1, None)                    # the initial step on blank from the zero state, into block 0
        lstm = dec.dtype == "lstm"
        layers = range(dec.dlayers)
        p = 0
        if frames:
            ft = self._frame_rows(hl, T, W, frames, levels=LV)          # the same rows for every history level
            ops.gather_rows([(ws["encr"], enc_rows, ft[0])])
        for t in range(frames):
            kp, ko = (N + 1, 0) if p else (0, N + 1)
            for v in range(1 if N == 1 else N + 1):
                last = N == 1 or v == N
                if v == 0 and alpha:
                    rec = ops.transducer_expand_rows_pairs_dev(jn.joint_rows_d(ws["encr"], hs[kp].view(LV * R, J)), k, ws["pairs"],
                                                               ws["pair_lp"])[:R]
                else:
                    rec = ops.transducer_expand_rows_dev(jn.joint_rows_d(ws["encr"][:R], hs[kp if v == 0 else v, 0]), k)
                ops.rnnt_nsc_step(rec, ws["pair_lp"], hl, st, ws["S"], ws["par"], ws["tok"], ws["live"], ws["hidx"], ws["pairs"],
                                  V, T, N, alpha, t, v, p)
                if last and t == frames - 1:
                    break                                      # the last kept's prediction state is never read
                cout = ko if last else v + 1
                step = N == 1 or not last                      # rows of the new block may have appended a token
                dst = 0 if step else 1
                jobs = [(blk[cout]["h"][dst][l], ws["h"][l], ws["par"]) for l in layers]
                if lstm:
                    jobs += [(blk[cout]["c"][dst][l], ws["c"][l], ws["par"]) for l in layers]
                jobs += [(hs[cout, a], hs_rows, ws["hidx"][a]) for a in range(1 if step else 0, LV)]
                if last:
                    jobs.append((ws["encr"], enc_rows, ft[t + 1]))
                ops.gather_rows(jobs)
                if step:
                    self._pred_step(blk[cout], 0, 1, ws["live"])
            p = 1 - p
        last = N + 1 if p else 0
        layout = self._block_layout(n, W, 1 + T * N)
        return _pack(layout, [st[0][last], st[2][last], st[1][last], st[3][last]]), layout
