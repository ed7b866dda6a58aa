"""CPU: the host side of gradient accumulation (--accum_steps; Engine.loss_and_grads(micro=(i, K))).

The grouping helper, the flag, the per-step protocol of the trainers (pretrain.run_micro_batches) against a fake engine in the style of
tests/test_parallel_cpu.py, and the engine's own bookkeeping -- which micro-batch may follow which, and when a gradient range is handed
to grad_hook -- on an Engine that is never bound to a device. There is no CPU product path: the one kernel these paths launch
(pb_accum_f32) is replaced by the torch expression it computes, as _TorchXfer does there; the kernel itself is tested on the GPU."""
import pytest
import torch

from pianobart_amd import ops
from pianobart_amd._lib import PBError
from pianobart_amd.finetune_generation import get_args_generation
from pianobart_amd.pretrain import get_args_pretrain, group_batches, run_micro_batches


def _torch_accum(dst, src, add=True):
    if add:
        dst.add_(src)
    else:
        dst.copy_(src)


# ---------------------------------------------------------------------------------------------------- grouping and the flag
def test_group_batches_keeps_order_and_ends_on_a_short_group():
    assert list(group_batches(range(5), 2)) == [[0, 1], [2, 3], [4]]
    assert list(group_batches(range(6), 3)) == [[0, 1, 2], [3, 4, 5]]
    assert list(group_batches(range(3), 1)) == [[0], [1], [2]]
    assert list(group_batches(range(2), 5)) == [[0, 1]]
    assert list(group_batches([], 4)) == []
    assert list(group_batches(iter('abc'), 2)) == [['a', 'b'], ['c']]            # any iterable, consumed once
    with pytest.raises(ValueError):
        list(group_batches(range(3), 0))


@pytest.mark.parametrize('parse', [get_args_pretrain, get_args_generation])
def test_accum_steps_flag(parse, capsys):
    assert parse([]).accum_steps == 1
    assert parse(['--accum_steps', '4']).accum_steps == 4
    for bad in ('0', '-2', 'x'):
        with pytest.raises(SystemExit) as e:
            parse(['--accum_steps', bad])
        assert e.value.code == 2
    assert '--accum_steps' in capsys.readouterr().err


# ---------------------------------------------------------------------------------------------------- the per-step protocol
class _FakeEngine:
    """loss_and_grads as the trainers see it: local counts into a buffer that count_hook may rewrite, 24 sums in a buffer that the next
    call overwrites."""

    def __init__(self):
        self.scal = torch.zeros(32)
        self.calls = []

    def loss_and_grads(self, enc16, dec16, tgt16, loss_mask, emask, dmask, train=True, count_hook=None, micro=None, **kw):
        sums, counts = self.scal[0:24], self.scal[24:32]
        counts.copy_(loss_mask.reshape(-1, 8).sum(0))
        if count_hook is not None:
            count_hook(counts)
        sums.copy_(torch.arange(24.0) * float(loss_mask.sum()))
        self.calls.append(dict(micro=micro, counts=counts.clone(), train=train, kw=kw))
        return sums


class _FakeReducer:
    """A second rank whose counts equal this one's: the exchange doubles."""

    def __init__(self):
        self.count_calls = 0

    def reduce_counts(self, c):
        self.count_calls += 1
        c.mul_(2)


def _batch(rows, S=6, seed=0):
    lm = (torch.rand(rows, S, generator=torch.Generator().manual_seed(seed)) < 0.5).float()[:, :, None].repeat(1, 1, 8)
    lm[0, 0] = 1
    return (None, None, None, lm, None, None)


@pytest.mark.parametrize('with_reducer', [False, True])
def test_every_micro_batch_is_normalised_by_the_counts_of_the_whole_step(monkeypatch, with_reducer):
    monkeypatch.setattr(ops, 'accum_f32', _torch_accum)
    eng, red = _FakeEngine(), (_FakeReducer() if with_reducer else None)
    micro = [_batch(2, seed=1), _batch(1, seed=2), _batch(3, seed=3)]
    local = [m[3].reshape(-1, 8).sum(0) for m in micro]
    total = sum(local).clone()
    assert not torch.equal(local[0], local[1])
    seen = []
    sums = run_micro_batches(eng, red, micro, total, torch.empty(24), before=seen.append, train=True, ids_checked=True)
    world = 2 if with_reducer else 1
    assert [c['micro'] for c in eng.calls] == [(0, 3), (1, 3), (2, 3)] and seen == [0, 1, 2]
    for c in eng.calls:
        assert torch.equal(c['counts'], world * sum(local)) and c['train'] is True and c['kw'] == {'ids_checked': True}
    assert torch.equal(sums, torch.arange(24.0) * float(sum(m[3].sum() for m in micro)))          # the 24 sums of the three calls, added
    if with_reducer:
        assert red.count_calls == 1                                                                # one count exchange per optimizer step


@pytest.mark.parametrize('with_reducer', [False, True])
def test_one_batch_is_the_call_without_accumulation(monkeypatch, with_reducer):
    def no_kernel(*a, **k):
        raise AssertionError('a step of one batch must not launch the accumulate kernel')
    monkeypatch.setattr(ops, 'accum_f32', no_kernel)
    eng, red = _FakeEngine(), (_FakeReducer() if with_reducer else None)
    b = _batch(2, seed=4)
    sums = run_micro_batches(eng, red, [b], None, None, train=False)
    assert eng.calls[0]['micro'] is None and sums.data_ptr() == eng.scal.data_ptr()
    assert torch.equal(eng.calls[0]['counts'], (2 if with_reducer else 1) * b[3].reshape(-1, 8).sum(0))
    assert red is None or red.count_calls == 1


# ---------------------------------------------------------------------------------------------------- the engine's bookkeeping
def _unbound_engine():
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    from tests.golden_util import load_vocab
    e2w, w2e = load_vocab()
    cfg = BartConfig(max_position_embeddings=16, d_model=32, encoder_layers=1, decoder_layers=2, encoder_ffn_dim=64, decoder_ffn_dim=64,
                     encoder_attention_heads=2, decoder_attention_heads=2, dropout=0.0)
    return PianoBartLM(PianoBart(cfg, e2w, w2e))._get_engine()


def test_micro_must_be_well_formed_and_in_sequence():
    eng = _unbound_engine()
    assert eng._check_micro(None, True) is None and eng._check_micro((0, 1), True) is None and eng._check_micro((0, 1), False) is None
    for bad in ((1, 1), (2, 2), (-1, 2), (0, 0), (0.5, 2), 3, (1, 2, 3), ('a', 2)):
        with pytest.raises(PBError):
            eng._check_micro(bad, True)
    with pytest.raises(PBError):
        eng._check_micro((0, 2), False)                      # accumulation belongs to training steps
    with pytest.raises(PBError, match='must follow'):
        eng._check_micro((1, 2), True)                       # no (0, 2) before it
    assert eng._check_micro((0, 3), True) == (0, 3)
    eng._micro_prev = (0, 3)                                  # what loss_and_grads leaves after micro-batch 0 of 3
    with pytest.raises(PBError, match='must follow'):
        eng._check_micro((1, 2), True)                       # another K
    eng._micro_prev = (0, 3)
    with pytest.raises(PBError, match='must follow'):
        eng._check_micro((2, 3), True)                       # skips micro-batch 1
    eng._micro_prev = (0, 3)
    assert eng._check_micro((1, 3), True) == (1, 3)
    assert eng.G_acc is None


def _ranges_of_a_backward(eng):
    """The calls Engine.backward and heads_backward make to declare gradient ranges final, in their order."""
    eng._ready('head.w')
    for l in reversed(range(eng.ND)):
        eng._ready('dec.%d.wqkv' % l, 'dec.%d.w2' % l)
    eng._ready('dec.wkv_all')
    for l in reversed(range(eng.NE)):
        eng._ready('enc.%d.wqkv' % l, 'enc.%d.w2' % l)
    eng._ready('emb', 'lin.w')


def test_gradient_ranges_reach_the_hook_once_per_step_and_summed(monkeypatch):
    """Engine._ready on host tensors: micro-batches before the last announce nothing; the last one adds G_acc to each range in front of
    its hook call, and the ranges are those of a step without accumulation."""
    monkeypatch.setattr(ops, 'accum_f32', _torch_accum)
    eng = _unbound_engine()
    n = eng.n_total
    eng.G32 = eng.Gcur = torch.arange(n, dtype=torch.float32)
    eng.G_acc = torch.full((n,), 0.5)
    seen = []
    eng.grad_hook = lambda lo, hi: seen.append((lo, hi, eng.G32[lo:hi].clone()))
    _ranges_of_a_backward(eng)                               # no accumulation: ranges as they are
    plain = [(lo, hi) for lo, hi, _ in seen]
    assert all(torch.equal(g, torch.arange(lo, hi, dtype=torch.float32)) for lo, hi, g in seen)
    assert sorted(plain)[0][0] == 0 and sum(hi - lo for lo, hi in plain) == eng.n_matrix            # the matrix region, each element once
    seen.clear()
    eng._micro = (0, 2)
    _ranges_of_a_backward(eng)
    assert seen == [] and torch.equal(eng.G32, torch.arange(n, dtype=torch.float32))
    eng._micro = (1, 2)
    _ranges_of_a_backward(eng)
    assert [(lo, hi) for lo, hi, _ in seen] == plain
    assert all(torch.equal(g, torch.arange(lo, hi, dtype=torch.float32) + 0.5) for lo, hi, g in seen)
    want = torch.arange(n, dtype=torch.float32)
    want[:eng.n_matrix] += 0.5
    assert torch.equal(eng.G32, want)                        # every range added exactly once; the vector region is the closing call's
