"""CER / WER during validation, scored on the device.

reference: espnet/nets/e2e_asr_common.py:103-402 (ErrorCalculator, ErrorCalculatorTransducer).  The reference copies the
id tensors to the host, joins Python strings and calls editdistance per utterance.  Here the string rules are compiled once
into token tables of Unicode code points; ops.text_units applies them to the id tensors and ops.edit_distance scores the
symbol rows, so per-utterance error counts and reference lengths exist as int32 device tensors (`counts`) and nothing is
read by the host until the caller wants the rate (`sums`, `__call__`).

The tables (CSR: tok_off [V+1], tok_cp, both int32):
  hyp  "".join(tokens).replace(space, " ").replace(blank, "")   space -> [0x20], blank -> nothing, others -> own code points
  ref  "".join(tokens).replace(space, " ")                      like hyp, but blank keeps its own code points
  ctc  calculate_cer_ctc drops the *ids* of blank and space     blank, space -> nothing, others -> own code points
A token table equals the string rules only while str.replace cannot match across a token boundary or inside another token.
The constructor checks what makes that certain and raises ValueError otherwise:
  * no token but sym_space contains a whitespace character (str.split() would split inside it, .replace(" ", "") would eat it);
  * neither sym_space nor sym_blank is a substring of another token;
  * no token (the symbols themselves included) ends with a non-empty proper prefix of sym_space or sym_blank: an occurrence
    of the symbol that is not a token of its own has to start inside some token and either end inside it (second check) or
    run over its end, and then that token ends with a proper prefix of the symbol (this check).
"""
import torch

from .. import ops


def _proper_prefixes(s):
    return [s[:k] for k in range(1, len(s))]


def check_token_list(char_list, sym_space, sym_blank):
    """ValueError unless the token tables reproduce the reference's string handling for every id sequence (module docstring)"""
    for tok in char_list:
        if tok != sym_space and any(c.isspace() for c in tok):
            raise ValueError("token %r contains whitespace: only sym_space %r may" % (tok, sym_space))
    for sym in (sym_space, sym_blank):
        if not sym:
            raise ValueError("empty sym_space / sym_blank")
        prefixes = _proper_prefixes(sym)
        for tok in char_list:
            if tok != sym and sym in tok:
                raise ValueError("token %r contains the symbol %r: str.replace would match inside it" % (tok, sym))
            for p in prefixes:
                if tok.endswith(p):
                    raise ValueError("token %r ends with %r, a prefix of the symbol %r: str.replace could match across "
                                     "tokens" % (tok, p, sym))


def build_table(char_list, empty=(), space=None):
    """CSR code-point table: ids in `empty` map to nothing, id `space` to [0x20], every other id to its token's code points.
    -> (tok_off list [V+1], tok_cp list, longest token)"""
    off, cp = [0], []
    for i, tok in enumerate(char_list):
        if i in empty:
            pass
        elif i == space:
            cp.append(0x20)
        else:
            cp.extend(ord(c) for c in tok)
        off.append(len(cp))
    longest = max([off[i + 1] - off[i] for i in range(len(char_list))] + [1])
    return off, cp, longest


class ErrorCalculator(object):
    """reference: e2e_asr_common.py:103-246; same constructor, same __call__ signature and return values"""

    def __init__(self, char_list, sym_space, sym_blank, report_cer=False, report_wer=False):
        self.report_cer = report_cer
        self.report_wer = report_wer
        self.char_list = list(char_list)
        self.space = sym_space
        self.blank = sym_blank
        self.idx_blank = self.char_list.index(self.blank)
        self.idx_space = self.char_list.index(self.space) if self.space in self.char_list else None
        check_token_list(self.char_list, sym_space, sym_blank)
        self.tables = dict(hyp=build_table(self.char_list, empty=(self.idx_blank,), space=self.idx_space),
                           ref=build_table(self.char_list, space=self.idx_space),
                           ctc=build_table(self.char_list, empty=(self.idx_blank, self.idx_space)))
        self._dev = None
        self._dev_tables = None

    def _tables_on(self, device):
        """the tables as device tensors: uploaded at the first call, and again only if the device changes"""
        if self._dev != device:
            self._dev_tables = {k: (ops.h2d_async(torch.tensor(off, dtype=torch.int32), device),
                                    ops.h2d_async(torch.tensor(cp or [0], dtype=torch.int32), device), longest)
                                for k, (off, cp, longest) in self.tables.items()}
            self._dev = device
        return self._dev_tables

    @staticmethod
    def _units(ids, table, limit=None, collapse=False, drop_cp=-1, mode=ops.TEXT_CHARS):
        off, cp, longest = table
        return ops.text_units(ids, off, cp, ids.shape[1] * longest, limit=limit, collapse=collapse, drop_cp=drop_cp, mode=mode)

    def counts(self, ys_hat, ys_pad, is_ctc=False):
        """ys_hat [B, Lh], ys_pad [B, L] integer id tensors on the GPU (-1 padding).
        is_ctc: -> (errors [B], ref_len [B]) int32 of calculate_cer_ctc; utterances with an empty reference count 0 errors.
        else:   -> (chars, words), each (errors [B], ref_len [B]) int32, or None where the report flag is off.
        Only kernels and tensor ops: nothing here reads from the device."""
        t = self._tables_on(ys_pad.device)
        hyp = ys_hat.to(torch.int32).contiguous()
        ref = ys_pad.to(torch.int32).contiguous()
        if is_ctc:
            h, hn = self._units(hyp, t["ctc"], collapse=True)
            r, rn = self._units(ref, t["ctc"])
            err = ops.edit_distance(h, hn, r, rn)
            return err * (rn > 0).to(torch.int32), rn            # `if len(ref_chars) > 0` as a mask
        # y_hat[:ymax], ymax = position of the first -1 of the reference row (its length when there is none)
        ymax = ((ref == -1).cumsum(1) == 0).sum(1).to(torch.int32)
        chars = words = None
        if self.report_cer:
            h, hn = self._units(hyp, t["hyp"], limit=ymax, drop_cp=0x20)
            r, rn = self._units(ref, t["ref"], drop_cp=0x20)
            chars = (ops.edit_distance(h, hn, r, rn), rn)
        if self.report_wer:
            h, hn = self._units(hyp, t["hyp"], limit=ymax, mode=ops.TEXT_WORDS)
            r, rn = self._units(ref, t["ref"], mode=ops.TEXT_WORDS)
            words = (ops.edit_distance(h, hn, r, rn), rn)
        return chars, words

    def counts_ctc_text(self, ys_hat, ys_pad):
        """the RNN E2E's greedy-CTC character errors (reference: e2e_asr.py:237-263): groupby over the frame argmax like
        calculate_cer_ctc, but the *text* rules of convert_to_char (space -> " ", blank removed, then " " removed), no ymax.
        -> (errors [B], ref_len [B]) int32; an empty reference counts 0 errors"""
        t = self._tables_on(ys_hat.device)
        h, hn = self._units(ys_hat.to(torch.int32).contiguous(), t["hyp"], collapse=True, drop_cp=0x20)
        r, rn = self._units(ys_pad.to(torch.int32).contiguous(), t["ref"], drop_cp=0x20)
        return ops.edit_distance(h, hn, r, rn) * (rn > 0).to(torch.int32), rn

    @staticmethod
    def sums(*counts):
        """[(errors, ref_len) or None, ...] -> [(sum errors, sum ref_len) as Python ints, or None, ...]: one host read"""
        live = [c for c in counts if c is not None]
        if not live:
            return [None for _ in counts]
        flat = torch.stack([torch.stack([e.sum(), n.sum()]) for e, n in live]).tolist()
        it = iter(flat)
        return [tuple(next(it)) if c is not None else None for c in counts]

    def __call__(self, ys_hat, ys_pad, is_ctc=False):
        """-> cer_ctc (None when no reference is non-empty) when is_ctc, else (cer, wer); the rates are
        float(sum errors) / sum ref_len from the integer sums, as the reference computes them"""
        if is_ctc:
            (e, n), = self.sums(self.counts(ys_hat, ys_pad, is_ctc=True))
            return float(e) / n if n > 0 else None
        if not self.report_cer and not self.report_wer:
            return None, None
        chars, words = self.sums(*self.counts(ys_hat, ys_pad))
        cer = float(chars[0]) / chars[1] if chars is not None else None
        wer = float(words[0]) / words[1] if words is not None else None
        return cer, wer


class ErrorCalculatorTransducer(object):
    """reference: e2e_asr_common.py:249-402.  Hypotheses from the greedy search (beam_size=1) on every hs_pad[b], all rows in one
    BeamSearchTransducer.greedy_batch call; their yseq[1:] are padded with -1, uploaded once and scored through ErrorCalculator's
    device path."""

    def __init__(self, decoder, token_list, sym_space, sym_blank, report_cer=False, report_wer=False):
        from .beam_search_transducer import BeamSearchTransducer
        self.beam_search = BeamSearchTransducer(decoder=decoder, beam_size=1)
        self.decoder = decoder
        self.token_list = token_list
        self.space = sym_space
        self.blank = sym_blank
        self.report_cer = report_cer
        self.report_wer = report_wer
        self.scorer = ErrorCalculator(token_list, sym_space, sym_blank, report_cer, report_wer)

    def hypotheses(self, hs_pad):
        """-> ys_hat [B, Lh] int32 on hs_pad's device, -1 padded"""
        # every padded row is decoded whole, as in the reference: all rows frame by frame in one batched greedy search
        ys_hat = [list(h.yseq[1:]) for h in self.beam_search.greedy_batch(hs_pad)]
        width = max(1, max(len(y) for y in ys_hat))
        host = torch.full((len(ys_hat), width), -1, dtype=torch.int32)
        for b, y in enumerate(ys_hat):
            host[b, : len(y)] = torch.tensor(y, dtype=torch.int32)
        return ops.h2d_async(host, hs_pad.device)

    def counts(self, hs_pad, ys_pad):
        return self.scorer.counts(self.hypotheses(hs_pad), ys_pad)

    def __call__(self, hs_pad, ys_pad):
        if not self.report_cer and not self.report_wer:
            return None, None
        return self.scorer(self.hypotheses(hs_pad), ys_pad)
