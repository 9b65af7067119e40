"""n-gram LM shallow fusion: ARPA back-off models as flat device tables, scored by one HIP launch per beam step.

reference: espnet/nets/scorers/ngram.py:12-102 (Ngrambase, NgramFullScorer, NgramPartScorer on kenlm),
espnet/asr/pytorch_backend/recog.py:68-87 (--ngram-model, --ngram-weight, --ngram-scorer {full,part}).

The reference asks kenlm for one (state, word) score per vocabulary entry, per hypothesis, per step.  A back-off model's row
over the whole vocabulary is a function of the last N - 1 words only:

    log10 p(w | h) = lp(h' w) + sum of backoff(h'') over the suffixes h'' of h that are longer than h',

h' being the longest suffix of h for which the n-gram (h' w) is listed.  `ArpaLM` reads the ARPA text itself (kenlm returns
exactly these numbers for a well-formed ARPA file: base-10 logs, which the reference passes on unconverted) and lays the
model out so that eamd_ngram_score (csrc/ngram.hip) writes the row as the dense unigram row plus a few sparse overwrites:

    tok2word [V]   token id -> LM word id ("<eos>" reads "</s>", ngram.py:23; a token the file does not list is <unk>)
    uni_tok  [V]   unigram log10-prob of tok2word[v], laid out by token id
    a trie of contexts stored MOST RECENT WORD FIRST: the node of the length-j suffix of a history is a child of the node of
    its length-(j-1) suffix, so the suffixes of one history are one root-to-leaf walk.  Node 0 is the empty context.
      node_bo     [M]            back-off weight of the context (0 for a context that only occurs inside a longer n-gram)
      child_start [M + 1]        edges of node m: child_word / child_node[child_start[m] : child_start[m + 1]], sorted by word
      succ_start  [M + 1]        n-grams that extend node m's context: succ_tok / succ_lp[succ_start[m] : succ_start[m + 1]],
                                 already expanded to token ids (a word several tokens map to: one entry per token; a word no
                                 token maps to: none).  The root's successors are the dense row uni_tok.
      qsucc_tok / qsucc_lp       the same ranges once more, sorted by token id inside a node: what a point query of one
                                 (context, token) pair bisects (eamd_ngram_score_pairs, the CTC prefix beam search)

The scorers' state is the context: int32 [N - 1] word ids, most recent first, -1 for an empty slot.
"""
import numpy as np
import torch

from .scorer_interface import BatchScorerInterface, PartialScorerInterface

MAX_ORDER = 8                      # csrc/ngram.hip keeps a walk of at most 7 context words
UNK_MISSING_LOGPROB = -100.0       # kenlm's default `unknown_missing_logprob` for a model without <unk> (lm/config.cc);
#                                    kenlm is not available to the tests, so this value is taken from its documentation

_TABLES = ("tok2word", "uni_tok", "node_bo", "child_start", "child_word", "child_node", "succ_start", "succ_tok", "succ_lp")
_QUERY_TABLES = ("qsucc_tok", "qsucc_lp")      # for point queries (csrc/ngram_query.h); eamd_ngram_score does not read them


def _parse_arpa(path):
    """-> (order, [dict word-tuple -> (log10 prob, back-off)] per order); ValueError with the line number when malformed"""
    counts, grams, section, seen_data, ended, ln = {}, {}, None, False, False, 0

    def bad(msg):
        return ValueError("%s:%d: %s" % (path, ln, msg))

    with open(path, encoding="utf-8") as f:
        for ln, raw in enumerate(f, 1):
            line = raw.strip()
            if not line:
                continue
            if ended:
                raise bad("text after \\end\\")
            if line.startswith("\\"):
                if line == "\\data\\":
                    if seen_data:
                        raise bad("second \\data\\ section")
                    seen_data, section = True, 0
                elif line == "\\end\\":
                    if not seen_data:
                        raise bad("\\end\\ before \\data\\")
                    ended = True
                elif line.endswith("-grams:"):
                    try:
                        k = int(line[1:-len("-grams:")])
                    except ValueError:
                        raise bad("unreadable section header %r" % line) from None
                    if k not in counts:
                        raise bad("section %r is not announced in \\data\\" % line)
                    if k != len(grams) + 1:
                        raise bad("section %r out of order" % line)
                    if k > 1 and len(grams[k - 1]) != counts[k - 1]:
                        raise bad("%d %d-grams announced, %d read" % (counts[k - 1], k - 1, len(grams[k - 1])))
                    section, grams[k] = k, {}
                else:
                    raise bad("unknown section %r" % line)
                continue
            if section is None:
                raise bad("text before \\data\\")
            if section == 0:
                if not line.startswith("ngram ") or "=" not in line:
                    raise bad("expected 'ngram K=COUNT'")
                try:
                    k, c = (int(v) for v in line[len("ngram "):].split("="))
                except ValueError:
                    raise bad("expected 'ngram K=COUNT'") from None
                if k != len(counts) + 1 or c < 0:
                    raise bad("orders must be announced as 1, 2, ... with counts >= 0")
                if k > MAX_ORDER:
                    raise NotImplementedError("%s: order %d (orders up to %d are supported)" % (path, k, MAX_ORDER))
                counts[k] = c
                continue
            cols = line.split()
            if len(cols) not in (section + 1, section + 2):
                raise bad("a %d-gram line has %d or %d columns" % (section, section + 1, section + 2))
            try:
                lp = float(cols[0])
                bo = float(cols[section + 1]) if len(cols) == section + 2 else 0.0      # the back-off column is optional
            except ValueError:
                raise bad("unreadable number") from None
            grams[section][tuple(cols[1:section + 1])] = (lp, bo)
    ln += 1
    if not seen_data or not ended:
        raise bad("file ends before \\end\\")
    order = len(counts)
    if order < 1 or len(grams) != order:
        raise bad("%d orders announced, %d sections read" % (order, len(grams)))
    if len(grams[order]) != counts[order]:
        raise bad("%d %d-grams announced, %d read" % (counts[order], order, len(grams[order])))
    return order, [grams[k] for k in range(1, order + 1)]


class ArpaLM:
    """a text ARPA file of order 1 <= N <= 8 as the flat tables of the module docstring (torch tensors; .to(device) moves them)"""

    def __init__(self, path, token_list):
        order, grams = _parse_arpa(path)
        self.order = order
        words = {w[0]: i for i, w in enumerate(grams[0])}
        uni_lp = [v[0] for v in grams[0].values()]
        if "<unk>" not in words:               # kenlm: a model without <unk> gives it unknown_missing_logprob, back-off 0
            words["<unk>"] = len(words)
            uni_lp.append(UNK_MISSING_LOGPROB)
        if "<s>" not in words:
            raise ValueError("%s: no <s> unigram" % path)
        self.words, self.bos, self.unk = words, words["<s>"], words["<unk>"]
        chardict = [x if x != "<eos>" else "</s>" for x in token_list]          # reference ngram.py:23
        V = len(chardict)
        tok2word = np.asarray([words.get(t, self.unk) for t in chardict], dtype=np.int32)
        uni_lp = np.asarray(uni_lp, dtype=np.float32)

        # ---- the context trie: one node per k-gram (k < N) and per context of a longer n-gram, keyed most recent word first
        nodes = {(): 0}
        levels = [[()]] + [[] for _ in range(order - 1)]

        def add(key):
            for j in range(1, len(key) + 1):
                if key[:j] not in nodes:
                    nodes[key[:j]] = -1
                    levels[j].append(key[:j])

        ids = [{g: tuple(words[w] for w in g) for g in grams[k] if all(w in words for w in g)} for k in range(order)]
        for k in range(order - 1):             # k + 1 words: a context with its own back-off weight
            for g in ids[k].values():
                add(g[::-1])
        for k in range(1, order):              # the context of every longer n-gram (back-off 0 unless listed itself)
            for g in ids[k].values():
                add(g[-2::-1])
        # ids level by level, the nodes of a level sorted by (parent, word): the children of a node are consecutive and sorted,
        # and edge e leads to node e + 1
        child_word, parent = [], []
        for j in range(1, order):
            keyed = sorted((nodes[key[:-1]], key[-1], key) for key in levels[j])
            for p, w, key in keyed:
                nodes[key] = len(child_word) + 1
                child_word.append(w)
                parent.append(p)
        M = len(child_word) + 1
        parent = np.asarray(parent, dtype=np.int64)
        child_start = np.searchsorted(parent, np.arange(M + 1)).astype(np.int32)
        node_bo = np.zeros(M, dtype=np.float32)            # (node 0, the empty context, has none: nothing is shorter)
        for k in range(order - 1):
            for g, wid in ids[k].items():
                node_bo[nodes[wid[::-1]]] = grams[k][g][1]

        # ---- successors: the n-grams of order >= 2 under the node of their context, expanded to token ids
        s_node, s_word, s_lp = [], [], []
        for k in range(1, order):
            for g, wid in ids[k].items():
                s_node.append(nodes[wid[-2::-1]])
                s_word.append(wid[-1])
                s_lp.append(grams[k][g][0])
        s_node, s_word = np.asarray(s_node, dtype=np.int64), np.asarray(s_word, dtype=np.int64)
        s_lp = np.asarray(s_lp, dtype=np.float32)
        by_word = np.argsort(tok2word, kind="stable").astype(np.int32)          # token ids grouped by word
        w_start = np.searchsorted(tok2word[by_word], np.arange(len(words) + 1))
        cnt = (w_start[1:] - w_start[:-1])[s_word] if len(s_word) else np.zeros(0, dtype=np.int64)
        rep = np.repeat(np.arange(len(s_word)), cnt)                            # entry of every (n-gram, token) pair
        within = np.arange(len(rep)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        s_tok = by_word[w_start[s_word[rep]] + within] if len(rep) else np.zeros(0, dtype=np.int32)
        o = np.argsort(s_node[rep], kind="stable")
        succ_start = np.searchsorted(s_node[rep][o], np.arange(M + 1)).astype(np.int32)

        def t(a, dtype):                       # (never empty: the entry point takes no NULL table)
            a = np.asarray(a, dtype=dtype)
            return torch.from_numpy(a.copy() if a.size else np.zeros(1, dtype=dtype))

        self.tok2word, self.uni_tok = t(tok2word, np.int32), t(uni_lp[tok2word], np.float32)
        self.node_bo, self.child_start = t(node_bo, np.float32), t(child_start, np.int32)
        self.child_word, self.child_node = t(child_word, np.int32), t(np.arange(1, M), np.int32)
        self.succ_start, self.succ_tok, self.succ_lp = t(succ_start, np.int32), t(s_tok[o], np.int32), t(s_lp[rep][o], np.float32)
        q = np.lexsort((s_tok[o], s_node[rep][o])) if len(rep) else np.zeros(0, dtype=np.int64)     # by node, then by token
        self.qsucc_tok, self.qsucc_lp = t(s_tok[o][q], np.int32), t(s_lp[rep][o][q], np.float32)
        self.n_vocab = V

    def to(self, device):
        for k in _TABLES + _QUERY_TABLES:
            setattr(self, k, getattr(self, k).to(device))
        return self

    @property
    def device(self):
        return self.uni_tok.device


class _NgramBase:
    """what the two scorers share: the tables (moved to the device of the first search), the start context, one row launch"""

    def __init__(self, ngram_model, token_list):
        self.lm = ngram_model if isinstance(ngram_model, ArpaLM) else ArpaLM(ngram_model, token_list)
        self.charlen = len(token_list)
        assert self.lm.n_vocab == self.charlen
        self._ctx0 = None

    def _start(self, device):
        """the context before <s>, [1, N - 1] of -1: allocated once per device (captured step graphs keep reading it)"""
        if self._ctx0 is None or self._ctx0.device != device:
            self.lm.to(device)
            self._ctx0 = torch.full((1, self.lm.order - 1), -1, dtype=torch.int32, device=device)
        return self._ctx0

    def init_state(self, x):
        self._start(x.device)
        return None                    # None = nothing scored yet: the first row is taken from the <s> context (ngram.py:50)

    def batch_init_state(self, x):
        return self.init_state(x)

    def final_score(self, state):
        return 0.0

    def _rows(self, ys, states):
        """ys [n, L] int64 prefixes on the device (L == 1: only <sos>, the newest word is <s>), states: [n, N - 1] contexts, a
        list of [N - 1] contexts, or None -> (rows [n, V], contexts [n, N - 1])"""
        from .. import ops
        first = ys.shape[1] == 1
        if states is None or first:
            ctx = self._start(ys.device).expand(ys.shape[0], -1)
        elif torch.is_tensor(states):
            ctx = states
        else:
            ctx = torch.stack(list(states))
        return ops.ngram_score(self.lm, ctx, ys[:, -1], first=first)


class NgramFullScorer(_NgramBase, BatchScorerInterface):
    """reference: scorers/ngram.py:60-77: for every token v, log10 p(word(v) | <s> + the prefix without its <sos>)"""

    def select_state(self, state, i, new_id=None):
        return None if state is None else state[i]

    def score(self, y, state, x):
        lp, ctx = self._rows(y.view(1, -1).to(x.device), None if state is None else state.view(1, -1))
        return lp[0], ctx[0]

    def batch_score(self, ys, states, xs):
        return self._rows(ys.to(xs.device), None if any(s is None for s in states) else states)

    def score_tree(self, ys, tree, xs):
        """the batched state is ONE bare tensor [n, N - 1] (BeamSearch._tree_index re-orders it with index_select; the one-graph
        steps decline a non-dict tree, so a search with this scorer keeps one graph per step).  No host synchronisation."""
        from .. import ops
        ctx = self._start(ys.device).expand(ys.shape[0], -1) if tree is None else tree
        return ops.ngram_score(self.lm, ctx, ys[:, -1], first=tree is None)

    def final_tree(self, tree):
        return 0.0


class NgramPartScorer(_NgramBase, PartialScorerInterface):
    """reference: scorers/ngram.py:80-102: the same row, gathered at the requested ids (host loop of BeamSearch only)"""

    def select_state(self, state, i, new_id=None):
        if state is None:
            return None
        return state[i[0] if isinstance(i, tuple) else i] if state.dim() == 2 else state     # (ngram.py:100-102: one state)

    def score_partial(self, y, next_tokens, state, x):
        lp, ctx = self._rows(y.view(1, -1).to(x.device), None if state is None else state.view(1, -1))
        return lp[0, next_tokens.to(lp.device).long()], ctx[0]

    def score_partial_batch(self, ys, ids, states, x=None):
        """ys [n, L], ids [n, P] -> (scores of ids [n, P], contexts [n, N - 1]); BeamSearch.search, "ids" mode"""
        lp, ctx = self._rows(ys, None if any(s is None for s in states) else states)
        return lp.gather(1, ids.long()), ctx


def build_ngram_scorer(recog_args, char_list):
    """reference: asr/pytorch_backend/recog.py:68-77 -> NgramFullScorer / NgramPartScorer of recog_args.ngram_model, or None"""
    path = getattr(recog_args, "ngram_model", None)
    if not path:
        return None
    kind = getattr(recog_args, "ngram_scorer", "part")
    if kind not in ("full", "part"):
        raise ValueError("ngram_scorer: 'full' or 'part', not %r" % (kind,))
    return (NgramFullScorer if kind == "full" else NgramPartScorer)(path, char_list)
