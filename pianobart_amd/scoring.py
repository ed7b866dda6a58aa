"""Teacher-forced scoring on the engine: what the model thinks of a GIVEN piece -- per token and head the log-probability of the piece's
event, the entropy of the head's distribution and the event's rank in it (pb_token_scores), and their per-sequence sums (pb_seq_scores).

ScoringMixin is the scoring part of pianobart_amd.engine.Engine, beside generation.GenerationMixin: it uses the engine's forward
schedule (forward_hidden, heads_forward) and id checks (bind, note_ids, check_ids) only, and nothing here imports engine.py. One
teacher-forced pass over all B * S decoder rows, dropout off; no decode path, nothing of the training step.

Reference semantics followed (file:line into the reference project): Ablation.py:126-166 -- the encoder sees a piece's first half, the
decoder is teacher-forced on the piece (input = the piece shifted right behind SOS) and its outputs are evaluated against the piece. The
reference does that inside a trainer, which stays out of scope; this is the forward-only quantity it evaluates.

The contract ("Scoring"):
  * target (B, S, 8): the piece as the decoder should emit it. Position i of row b is scored iff start_b <= i < length_b.
  * decoder input = pb_shift_right(target, SOS); decoder attention mask of row b = 1 on positions 0 .. max(length_b - 1, 0)
    (position 0 is always on, as in the generate loop).
  * a position that is not scored gives logp = 0, entropy = 0, rank = -1 and adds nothing to the sums.
"""
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from ._lib import PBError


def _int_list(v):
    return [int(x) for x in (v.tolist() if hasattr(v, 'tolist') else list(v))]


def default_length(target_ids, bar_pad):
    """length_b of a (B, S, 8) piece array (tensor on any device, or array): the number of LEADING rows whose bar id is not the bar PAD --
    for a row of generate_batch its emitted length (the result is PAD behind the stop)."""
    t = torch.as_tensor(target_ids)
    live = (t[:, :, 0] != int(bar_pad)).to(torch.int64)
    return _int_list(live.cumprod(1).sum(1))


def check_score_args(input_ids_encoder, target_ids, start=None, length=None, max_positions=None, bar_pad=None):
    """The argument rules of scoring, on the host before any device work: both id tensors (B, S, 8) with equal B and S and an integer
    dtype, S <= max_positions, start / length B ints with 0 <= start_b <= length_b <= S. Defaults: start_b = 0, length_b =
    default_length(target_ids, bar_pad). Returns (start, length) as lists of B ints. Raises PBError."""
    e, t = torch.as_tensor(input_ids_encoder), torch.as_tensor(target_ids)
    for name, x in (('input_ids_encoder', e), ('target_ids', t)):
        if x.dim() != 3 or int(x.shape[2]) != 8:
            raise PBError('score: %s of shape %s: expected (B, S, 8)' % (name, tuple(x.shape)))
        if x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool:
            raise PBError('score: %s must hold integers (got %s)' % (name, x.dtype))
    if tuple(e.shape) != tuple(t.shape):
        raise PBError('score: input_ids_encoder %s and target_ids %s must have the same (B, S, 8)' % (tuple(e.shape), tuple(t.shape)))
    B, S = int(t.shape[0]), int(t.shape[1])
    if max_positions is not None and S > int(max_positions):
        raise PBError('score: sequence length %d exceeds max_position_embeddings %d' % (S, int(max_positions)))
    if length is None:
        if bar_pad is None:
            raise PBError('score: the default length needs the bar PAD id')
        length = default_length(t, bar_pad)
    start = [0] * B if start is None else start
    out = []
    for name, v in (('start', start), ('length', length)):
        try:
            vals = v.tolist() if hasattr(v, 'tolist') else list(v)
        except TypeError:
            raise PBError('score: %s must be a sequence of %d ints (got %r)' % (name, B, v))
        if len(vals) != B:
            raise PBError('score: %s has %d entries for %d row(s)' % (name, len(vals), B))
        for b, x in enumerate(vals):
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
                raise PBError('score: %s[%d] = %r is not an integer' % (name, b, x))
        out.append([int(x) for x in vals])
    start, length = out
    for b in range(B):
        if not 0 <= start[b] <= length[b] <= S:
            raise PBError('score: row %d: start = %d, length = %d outside 0 <= start <= length <= %d' % (b, start[b], length[b], S))
    return start, length


def pick_best(scores):
    """--pick best of eval_generation as a pure numpy helper. scores (N, n, 9) = per sample the 8 per-head sum_logp and the count of scored
    positions. Returns (N,) int64: per prompt the sample with the largest sum_heads(sum_logp) / count; samples with count == 0 rank last;
    ties go to the lower sample index."""
    s = np.asarray(scores, dtype=np.float64)
    if s.ndim != 3 or s.shape[2] != 9:
        raise PBError('pick_best: scores of shape %s: expected (N, n, 9)' % (s.shape,))
    total, count = s[:, :, :8].sum(-1), s[:, :, 8]
    with np.errstate(divide='ignore', invalid='ignore'):
        key = np.where(count > 0, total / np.where(count > 0, count, 1.0), -np.inf)
    return np.argmax(key, axis=1).astype(np.int64)             # np.argmax: the first maximum


class ScoringMixin:
    def score(self, enc16, tgt16, emask, start, length):
        """Teacher-forced scores of B pieces. enc16 / tgt16 (B, S, 8) int16 device, emask (B, S) or None, start / length: B ints with
        0 <= start_b <= length_b <= S (check_score_args). Returns a SimpleNamespace of device tensors: logp, entropy (B, S, 8) f32, rank
        (B, S, 8) int16, sum_logp, sum_entropy, hits (B, 8) f32 and count (B,) f32 (module docstring). Raises IndexError for an id outside
        its embedding table (special ids are legal targets). All B * S decoder rows are computed; dropout is off; apart from the
        activation workspace, which every forward overwrites, nothing is written that a later training step reads."""
        if self.mlm is None:
            raise PBError('engine has no LM heads')
        if enc16.device.type != 'cuda':
            raise PBError('pianobart_amd needs HIP device tensors (got %s); there is no CPU path' % enc16.device)
        B, S = int(tgt16.shape[0]), int(tgt16.shape[1])
        start, length = _int_list(start), _int_list(length)
        if len(start) != B or len(length) != B or any(not 0 <= s <= n <= S for s, n in zip(start, length)):
            raise PBError('score: start / length need %d entries with 0 <= start <= length <= %d' % (B, S))
        dev = enc16.device
        self.bind(dev)
        self._await_updates(2)
        with torch.no_grad():
            enc16 = self.note_ids(enc16.contiguous(), owned=False)
            tgt16 = self.note_ids(tgt16.contiguous(), owned=False)
            em = emask.to(torch.float32).contiguous() if emask is not None else None
            pos = torch.arange(S, device=dev).unsqueeze(0)
            st = torch.tensor(start, device=dev).unsqueeze(1)
            ln = torch.tensor(length, device=dev).unsqueeze(1)
            mask = ((pos >= st) & (pos < ln)).to(torch.float32).contiguous()
            dmask = (pos < ln.clamp(min=1)).to(torch.float32).contiguous()
            dec16 = torch.empty_like(tgt16)
            ops.shift_right(tgt16, self.sos16, dec16, B, S)
            dec_h, _ = self.forward_hidden(enc16, dec16, em, dmask, False, 0)
            logits = self.heads_forward(dec_h)
            logp = torch.empty(B, S, 8, dtype=torch.float32, device=dev)
            entropy = torch.empty(B, S, 8, dtype=torch.float32, device=dev)
            rank = torch.empty(B, S, 8, dtype=torch.int16, device=dev)
            sums = torch.empty(B, 4, 8, dtype=torch.float32, device=dev)
            ops.token_scores(logits, tgt16.view(B * S, 8), mask.view(B * S), logp, entropy, rank, layout=self.lay)
            ops.seq_scores(logp, entropy, rank, mask, sums)
        self.check_ids(collective=False)          # a rank may score by itself: local verdict (synchronises; an offending id was read as 0)
        return SimpleNamespace(logp=logp, entropy=entropy, rank=rank, sum_logp=sums[:, 0], sum_entropy=sums[:, 1], hits=sums[:, 2],
                               count=sums[:, 3, 0])
