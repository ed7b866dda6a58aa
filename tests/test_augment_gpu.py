"""GPU: pb_augment and the trainers' use of it, against the numpy restatement tests/augment_ref.py. Integer work: every comparison is ==.

Shapes: S covers one partial pass of the 256-thread workgroup (1, 7, 8, 63 .. 65), exactly one pass and its neighbours (255, 256, 257), whole
multiples (1024, 2048) and one past (2049); the kernel re-reads the rows at every S, so there is no second code path to reach. B = 1, 3, 17.
The trainers run a 2 + 2 layer model (d = 256, 4 heads) at S = 64."""
import ctypes

import numpy as np
import pytest
import torch

from pianobart_amd import augment, ops
from pianobart_amd._lib import LIB, PBError
from tests import augment_ref as R
from tests.golden_util import load_vocab, synth_octuple_batch
from tests.test_augment_cpu import _pieces, draw_cases
from tests.vocab_layout_util import D_WIDE, make_dict

gpu = pytest.mark.gpu
FIXED = [0, 1, 2, 4, 6]                       # the heads no axis owns
_CACHE = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _dev(ids):
    return torch.from_numpy(np.ascontiguousarray(ids)).to(torch.int16).cuda()


def _run(ids, plan, seed, inplace=False):
    """(out, shifts) of augment.apply as int64 arrays; the input tensor must come back unchanged from the out-of-place call."""
    x = _dev(ids)
    out, s = augment.apply(x, plan, seed, out=x if inplace else None)
    torch.cuda.synchronize()
    if not inplace:
        assert out.data_ptr() != x.data_ptr() and torch.equal(x.cpu(), torch.from_numpy(np.asarray(ids)).to(torch.int16))
    return out.cpu().numpy().astype(np.int64), s.cpu().numpy().astype(np.int64)


def _check(ids, plan, seed):
    """The kernel against the reference, out of place and in place; returns (out, shifts)."""
    want, ws = R.reference(ids, plan.coord, plan.id_at, plan.plan, seed)
    out, s = _run(ids, plan, seed)
    assert (s == ws).all() and (out == want).all()
    assert (out[:, :, FIXED] == np.asarray(ids)[:, :, FIXED]).all()
    out2, s2 = _run(ids, plan, seed, inplace=True)
    assert (out2 == want).all() and (s2 == ws).all()
    return out, s


def _plan(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _CACHE:
        _CACHE[key] = augment.AugmentPlan(None, **kw)
    return _CACHE[key]


ALL3 = dict(pitch=(-6, 5), velocity=(-2, 2), tempo=(-2, 2))


# ---------------------------------------------------------------------------------------------------- sizes
@gpu
@pytest.mark.parametrize('S', [1, 7, 8, 63, 64, 65, 255, 256, 257, 1024, 2048, 2049])
def test_every_length_and_batch(S):
    _need_gpu()
    rng = np.random.default_rng(S)
    for B in (1, 3, 17):
        ids = _pieces(rng, B, S)
        ids[0, S - 1] = [3, 5, 0, 40, 9, 16, 8, 24]                 # the last position of a piece counts: an ordinary row there
        out, s = _check(ids, _plan(pitch_bounds=(0, 127), **ALL3), 1000 * S + B)
        if B == 17:
            assert (s != 0).any(axis=0).all() and (out != ids).any()


@gpu
def test_the_last_row_alone_sets_the_extremes():
    """A piece whose only high and only low note sit in the last rows of the last partial pass: a lane that dropped them would let the
    piece leave the axis."""
    _need_gpu()
    for S in (257, 2049):
        ids = np.zeros((2, S, 8), dtype=np.int64)
        ids[:, :, 3], ids[:, :, 5], ids[:, :, 7] = 60, 16, 24
        ids[0, S - 1, 3], ids[1, S - 1, 3] = 126, 2
        ids[0, S - 2, 5], ids[1, S - 2, 7] = 31, 0
        for seed in range(6):
            out, s = _check(ids, _plan(**ALL3), seed)
            assert -6 <= s[0, 0] <= 1 and -2 <= s[1, 0] <= 5 and s[0, 1] <= 0 and s[1, 2] >= 0


# ---------------------------------------------------------------------------------------------------- row kinds
@gpu
def test_row_kinds():
    _need_gpu()
    S = 16
    pad, n = np.asarray(ops.DEFAULT_LAYOUT.pad8), np.asarray(ops.DEFAULT_LAYOUT.sizes)
    note = np.array([1, 4, 0, 60, 8, 16, 8, 24])
    ids = np.tile(pad, (10, S, 1)).astype(np.int64)                                     # 0: all PAD
    ids[1, :9] = note; ids[1, :9, 3] = 128 + np.arange(9) * 13                          # 1: only percussion pitches
    ids[2, 0] = note                                                                    # 2: a single note
    ids[3, :5] = note; ids[3, :5, 3] = [0, 4, 7, 12, 16]; ids[3, :5, 5] = [0, 3, 5, 7, 9]; ids[3, :5, 7] = [0, 1, 2, 3, 4]        # 3: cmin = 0
    ids[4, :5] = note; ids[4, :5, 3] = [127, 120, 115, 110, 111]; ids[4, :5, 5] = [31, 30, 29, 28, 27]; ids[4, :5, 7] = [48, 40, 41, 42, 43]   # 4: cmax = ncoord - 1
    ids[5, :4] = note; ids[5, :4, 3] = [21, 60, 108, 64]                                # 5: the span equals the bounds
    ids[6, :4] = note; ids[6, :4, 3] = [20, 60, 70, 64]                                 # 6: a note below the bounds
    ids[7, :4] = note; ids[7, :4, 3] = [30, 60, 109, 64]                                # 7: a note above the bounds
    ids[8, :9] = note; ids[8, :9, 3] = 50 + np.arange(9)                                # 8: MASK / SOS / EOS rows between the notes
    ids[8, 2], ids[8, 5], ids[8, 7] = pad + 1, pad + 2, pad + 3
    ids[9, :S] = note; ids[9, :, 3] = np.where(np.arange(S) % 2, 128 + np.arange(S), 40 + np.arange(S))     # 9: notes and percussion mixed
    assert (ids < n).all()
    bounded, free = _plan(pitch_bounds=(21, 108), **ALL3), _plan(**ALL3)
    seen = [set() for _ in range(10)]
    for seed in range(12):
        out, s = _check(ids, bounded, seed)
        for b in range(10):
            seen[b].add(int(s[b, 0]))
        assert (out[0] == ids[0]).all() and (s[0] == 0).all()
        for b in (1, 5, 6, 7):                                                          # (their dynamics and tempo move as anyone's)
            assert (out[b, :, 3] == ids[b, :, 3]).all() and s[b, 0] == 0
        special = [2, 5, 7]
        assert (out[8, special] == ids[8, special]).all() and (out[8, 9:] == ids[8, 9:]).all()
        assert (out[9, 1::2, 3] == ids[9, 1::2, 3]).all()                               # percussion stays, the notes beside it move
        assert (out[9, 0::2, 3] == ids[9, 0::2, 3] + s[9, 0]).all()
        assert (out[2, 0, [3, 5, 7]] == ids[2, 0, [3, 5, 7]] + s[2]).all()
        out, s = _check(ids, free, seed)
        assert (s[3] >= 0).all() and (s[4] <= 0).all()                                  # no way down from 0, no way up from the top
    for b in (2, 8, 9):                                                                 # (that every value is drawn: the width test below)
        assert seen[b] <= set(range(-6, 6)) and len(seen[b]) > 3
    assert seen[5] == seen[6] == seen[7] == {0}


# ---------------------------------------------------------------------------------------------------- draws
@gpu
def test_draws_are_the_references_at_every_width():
    _need_gpu()
    for w, ids, plan in draw_cases():                               # w = 1 .. 12, 4096 pieces each; w = 1 forces s = lo = 0
        want, ws = R.reference(ids, plan.coord, plan.id_at, plan.plan, 0xA5A5 + w)
        out, s = _run(ids, plan, 0xA5A5 + w)
        assert (s == ws).all() and (out == want).all()
        assert sorted(set(s[:, 0].tolist())) == list(range(int(plan.plan[0][0]), int(plan.plan[0][1]) + 1))


@gpu
@pytest.mark.parametrize('axes', [('pitch',), ('velocity',), ('tempo',), ('pitch', 'velocity', 'tempo')])
@pytest.mark.parametrize('prob', [1.0, 0.5, 0.05])
def test_axes_alone_and_together_with_prob(axes, prob):
    _need_gpu()
    ids = _pieces(np.random.default_rng(11), 256, 33)
    plan = _plan(prob=prob, **{a: ALL3[a] for a in axes})
    out, s = _check(ids, plan, 4242)
    off = [a for a, n in enumerate(augment.AXES) if n not in axes]
    assert (s[:, off] == 0).all() and (out[:, :, [R.HEADS[a] for a in off]] == ids[:, :, [R.HEADS[a] for a in off]]).all()
    on = [a for a, n in enumerate(augment.AXES) if n in axes]
    assert (s[:, on] != 0).any()
    if prob < 1:                                                    # untouched pieces are exactly the reference's
        _, full = R.reference(ids, plan.coord, plan.id_at, _plan(**{a: ALL3[a] for a in axes}).plan, 4242)
        assert ((s == 0) | (s == full)).all() and ((s == 0) & (full != 0)).any()


@gpu
def test_seeds_and_determinism():
    _need_gpu()
    ids = _pieces(np.random.default_rng(12), 17, 100)
    plan = _plan(**ALL3)
    a, sa = _run(ids, plan, 5)
    b, sb = _run(ids, plan, 5)
    c, sc = _run(ids, plan, 6)
    assert (a == b).all() and (sa == sb).all()
    assert (a != c).any() and (sa != sc).any()
    hi, _ = _check(ids, plan, (1 << 63) + 5)                        # the high half of the seed is part of the key
    assert (hi != a).any()


# ---------------------------------------------------------------------------------------------------- another dictionary
@gpu
def test_wide_dictionary():
    _need_gpu()
    e2w, _ = make_dict(D_WIDE)                                      # pitch head: 512 ordinary classes
    plan = augment.AugmentPlan(e2w, pitch=(-40, 40), velocity=(-3, 3), tempo=(-5, 5), pitch_bounds=(10, 500))
    rng = np.random.default_rng(13)
    ids = _pieces(rng, 17, 70, D_WIDE)
    for b in range(17):                                             # pitches over the whole wide head
        lo = rng.integers(0, 400)
        ids[b, :, 3] = np.where(ids[b, :, 3] < 512, rng.integers(lo, lo + 100, size=70), ids[b, :, 3])
    out, s = _check(ids, plan, 77)
    assert np.abs(s[:, 0]).max() > 6 and (out[:, :, 3] >= 272).any()


# ---------------------------------------------------------------------------------------------------- refusals
@gpu
def test_entry_refusals_leave_out_unchanged():
    _need_gpu()
    B, S = 2, 9
    plan = _plan(**ALL3)
    ids = _dev(_pieces(np.random.default_rng(14), B, S))
    out = torch.full_like(ids, -7)
    shifts = torch.full((B, 3), -7, dtype=torch.int32, device='cuda')
    coord, id_at = plan.tables(ids.device)
    good = list(plan._plan18)

    def call(ids=ids, out=out, shifts=shifts, B=B, S=S, coord=coord, id_at=id_at, plan18=good):
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        rc = LIB.query('pb_augment', p(ids), p(out), p(shifts), B, S, p(coord), p(id_at), (ctypes.c_int32 * 18)(*plan18), ctypes.c_uint64(1),
                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc, LIB.query('pb_last_error').decode()

    def edited(axis, *pairs):
        q = list(good)
        for field, value in pairs:
            q[6 * axis + field] = value
        return q

    cases = [(dict(ids=None), 'NULL'), (dict(out=None), 'NULL'), (dict(shifts=None), 'NULL'), (dict(coord=None), 'NULL'), (dict(id_at=None), 'NULL'),
             (dict(B=0), 'B=0'), (dict(B=65536), 'B=65536'), (dict(S=0), 'S=0'), (dict(S=65537), 'S=65537'),
             (dict(plan18=edited(0, (0, 1))), 'pitch'), (dict(plan18=edited(1, (1, -1))), 'velocity'), (dict(plan18=edited(2, (0, 3))), 'tempo'),
             (dict(plan18=edited(0, (2, -1))), 'bounds'), (dict(plan18=edited(0, (3, 128))), 'bounds'), (dict(plan18=edited(1, (2, 9), (3, 8))), 'bounds'),
             (dict(plan18=edited(2, (4, 0))), 'ncoord'), (dict(plan18=edited(2, (4, 1089))), 'ncoord')]
    flat = torch.zeros(B * S * 8 + 8, dtype=torch.int16, device='cuda')
    cases.append((dict(ids=flat[:B * S * 8], out=flat[8:]), 'overlaps'))
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc < 0 and 'pb_augment' in msg and word in msg, (kw.keys(), rc, msg)
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((shifts == -7).all()) and bool((flat == 0).all())
    rc, _ = call()
    assert rc == 0
    torch.cuda.synchronize()
    assert bool((shifts != -7).all())
    # the host side refuses before the entry is reached
    with pytest.raises(PBError, match='int16'):
        augment.apply(ids.long(), plan, 1)
    with pytest.raises(PBError, match='HIP device tensors'):
        augment.apply(ids.cpu(), plan, 1)
    with pytest.raises(PBError, match='out must match'):
        augment.apply(ids, plan, 1, out=torch.empty(B, S + 1, 8, dtype=torch.int16, device='cuda'))


# ---------------------------------------------------------------------------------------------------- trainers
S_T, B_T = 64, 4
_KW = dict(max_position_embeddings=S_T, d_model=256, encoder_layers=2, decoder_layers=2, encoder_ffn_dim=512, decoder_ffn_dim=512,
           encoder_attention_heads=4, decoder_attention_heads=4, dropout=0.0)


def _pretrainer(loader=None):
    from pianobart_amd.model import BartConfig, PianoBart
    from pianobart_amd.pretrain import Pretrainer
    from tests.golden_util import randomize_params
    e2w, w2e = load_vocab()
    torch.manual_seed(0)
    tr = Pretrainer(PianoBart(BartConfig(**_KW), e2w, w2e), loader, loader, 1e-4, B_T, S_T, 0.15, False, [0])
    randomize_params(tr.model, 5)
    tr.engine.bind(tr.device)
    tr.engine.refresh_shadow(force=True)
    tr.quiet = True
    return tr


def _loader(n=2):
    return [synth_octuple_batch(B_T, S_T, seed=40 + i)[5] for i in range(n)]


def _record(tr):
    """Every prepare_batch call of the trainer: (its augment seed, its tgt16, the shifts)."""
    seen, orig = [], tr.prepare_batch

    def prepare(batch, **kw):
        tr.last_shifts = None
        out = orig(batch, **kw)
        seen.append((kw.get('augment_seed'), out[2].cpu().numpy().astype(np.int64),
                     None if tr.last_shifts is None else tr.last_shifts.cpu().numpy().astype(np.int64)))
        return out

    tr.prepare_batch = prepare
    return seen


@gpu
def test_pretrainer_prepare_batch_off_and_on():
    _need_gpu()
    import random
    tr = _CACHE.setdefault('pretrainer', _pretrainer())
    tr.augment = None
    batch = _loader(1)[0]
    pb = tr.pianobart
    # off: what the existing path computes -- the same choices, the same step seed, pb_corrupt and pb_shift_right on the loader's rows
    for with_plan_but_no_seed in (False, True):
        tr.augment = _plan(**ALL3) if with_plan_but_no_seed else None
        random.seed(7)
        seed0 = tr._step_seed
        enc16, dec16, tgt16, lm, emask, dmask = tr.prepare_batch(batch)
        random.seed(7)
        choices = [random.randint(1, 5) for _ in range(B_T)]
        want_tgt = ops.ids_to_i16(batch.cuda())
        assert torch.equal(tgt16, want_tgt)
        enc_w, lm_w = torch.empty_like(want_tgt), torch.empty(B_T, S_T, 8, device='cuda')
        ops.corrupt(want_tgt, enc_w, lm_w, torch.tensor(choices, dtype=torch.int32, device='cuda'), None, 0.15,
                    (seed0 * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF, pb.pad_word_np, pb.mask_word_np, pb.n_tokens)
        dec_w = torch.empty_like(want_tgt)
        ops.shift_right(want_tgt, tr.engine.sos16, dec_w, B_T, S_T)
        assert torch.equal(enc16, enc_w) and torch.equal(lm, lm_w) and torch.equal(dec16, dec_w)
        assert torch.equal(emask, (enc_w[:, :, 0] != 256).float()) and torch.equal(dmask, (dec_w[:, :, 0] != 256).float())
    # on: the target is the reference's augmentation of the loader's rows, and everything else derives from it
    plan = tr.augment = _plan(**ALL3)
    seed = augment.batch_seed(3, 0, 2, 5)
    orig_choice = random.randint
    try:
        random.randint = lambda a, b: 2                             # every row takes TokenMask: positions stay where they are
        enc16, dec16, tgt16, lm, emask, dmask = tr.prepare_batch(batch, augment_seed=seed)
    finally:
        random.randint = orig_choice
    want, ws = R.reference(batch.numpy(), plan.coord, plan.id_at, plan.plan, seed)
    assert (ws != 0).any() and (want != batch.numpy()).any()
    assert (tgt16.cpu().numpy() == want).all() and (tr.last_shifts.cpu().numpy() == ws).all()
    dec_w = torch.empty_like(tgt16)
    ops.shift_right(tgt16, tr.engine.sos16, dec_w, B_T, S_T)
    assert torch.equal(dec16, dec_w) and torch.equal(dec16[:, 1:], tgt16[:, :-1])
    keep = lm[:, :, 0] == 0
    assert bool(keep.any()) and bool((~keep).any()) and torch.equal(enc16[keep], tgt16[keep])
    assert torch.equal(batch, _loader(1)[0])                        # the loader's batch is not written
    tr.augment = None


@gpu
def test_pretrainer_epochs_ranks_and_validation(monkeypatch):
    _need_gpu()
    loader = _loader(2)
    plan = _plan(**ALL3)
    want16 = [ops.ids_to_i16(b.cuda()).cpu().numpy().astype(np.int64) for b in loader]

    def run_epochs(tr, n):
        tr.train_data = tr.valid_data = loader
        tr.augment, tr.augment_seed = plan, 9
        seen = _record(tr)
        per_epoch = []
        for _ in range(n):
            del seen[:]
            tr.train()
            per_epoch.append(list(seen))
        return seen, per_epoch

    a = _CACHE.setdefault('pretrainer', _pretrainer())
    a._epoch = 0
    seen, ep = run_epochs(a, 2)
    for e in range(2):
        assert len(ep[e]) == 2
        for i, (seed, tgt, s) in enumerate(ep[e]):
            assert seed == augment.batch_seed(9, 0, e, i)
            want, ws = R.reference(want16[i], plan.coord, plan.id_at, plan.plan, seed)
            assert (tgt == want).all() and (s == ws).all()
    assert any((ep[0][i][2] != ep[1][i][2]).any() for i in range(2))            # a new epoch, new shifts
    # validation, and anything with train=False, sees the loader's rows
    del seen[:]
    a.valid()
    a.iteration(loader, S_T, train=False)
    assert len(seen) == 4
    for k, (seed, tgt, s) in enumerate(seen):
        assert seed is None and s is None and (tgt == want16[k % 2]).all()
    del a.prepare_batch
    a.augment = None
    # a trainer built for rank 1 draws other shifts
    monkeypatch.setenv('RANK', '1')
    b = _pretrainer()
    monkeypatch.delenv('RANK')
    assert b.rank == 1
    _, ep_b = run_epochs(b, 1)
    assert [x[0] for x in ep_b[0]] == [augment.batch_seed(9, 1, 0, i) for i in range(2)]
    assert any((ep_b[0][i][2] != ep[0][i][2]).any() for i in range(2))
    # a trainer that starts at epoch 1 (what resume() sets) draws what the first one drew at epoch 1
    b.rank, b._epoch = 0, 1
    del b.prepare_batch
    _, ep_c = run_epochs(b, 1)
    for i in range(2):
        assert ep_c[0][i][0] == ep[1][i][0] and (ep_c[0][i][2] == ep[1][i][2]).all() and (ep_c[0][i][1] == ep[1][i][1]).all()


@gpu
def test_generation_trainer_shifts_prompt_and_continuation_alike():
    _need_gpu()
    from pianobart_amd.finetune_generation import GenerationTrainer
    from pianobart_amd.model import BartConfig, PianoBart
    from tests.golden_util import randomize_params
    e2w, w2e = load_vocab()
    x, y = synth_octuple_batch(B_T, S_T, seed=50)[5], synth_octuple_batch(B_T, S_T, seed=51)[5]
    tr = GenerationTrainer(PianoBart(BartConfig(**_KW), e2w, w2e), [(x, y)], [(x, y)], [(x, y)], 1e-4, (B_T, S_T, 8), False, [0])
    randomize_params(tr.model, 13)
    tr.engine.bind(tr.device)
    plan = tr.augment = _plan(**ALL3)
    tr.augment_seed = 21
    seed = augment.batch_seed(21, 0, 0, 0)
    x16, y16, s = tr.augment_pair(ops.ids_to_i16(x.cuda()), ops.ids_to_i16(y.cuda()), seed)
    both = np.concatenate([x.numpy(), y.numpy()], axis=1)
    want, ws = R.reference(both, plan.coord, plan.id_at, plan.plan, seed)
    assert (s.cpu().numpy() == ws).all() and (ws != 0).any()
    assert (x16.cpu().numpy() == want[:, :S_T]).all() and (y16.cpu().numpy() == want[:, S_T:]).all()
    # each half carries the same shifts
    assert (x16.cpu().numpy() == R.apply_shifts(x.numpy(), plan.coord, plan.id_at, plan.plan, ws)).all()
    assert (y16.cpu().numpy() == R.apply_shifts(y.numpy(), plan.coord, plan.id_at, plan.plan, ws)).all()
    # the training iteration uses it with the batch's seed; validation does not
    seen, orig = [], tr.augment_pair
    tr.augment_pair = lambda *a: seen.append(a[2]) or orig(*a)
    tr.train()
    tr.valid()
    tr.train()
    assert seen == [augment.batch_seed(21, 0, 0, 0), augment.batch_seed(21, 0, 1, 0)]
    assert (tr.last_shifts.cpu().numpy() == R.shifts_of(both, plan.coord, plan.plan, seen[1])).all()


@gpu
def test_finetune_trainer_augments_training_batches_only():
    _need_gpu()
    from torch.utils.data import DataLoader
    from pianobart_amd.finetune import FinetuneDataset, FinetuneTrainer
    from pianobart_amd.model import BartConfig, PianoBart
    e2w, w2e = load_vocab()
    X = synth_octuple_batch(8, S_T, seed=3)[5].numpy()
    y = np.random.default_rng(0).integers(0, 8, size=(8,))
    mk = lambda: DataLoader(FinetuneDataset(X, y), batch_size=4)
    torch.manual_seed(0)
    pb = PianoBart(BartConfig(**_KW), e2w, w2e, precision='fp32')
    tr = FinetuneTrainer(pb, mk(), mk(), mk(), lr=1e-4, class_num=8, hs=256, testset_shape=y.shape, cpu=False, cuda_devices=[0], SeqClass=True)
    plan = tr.augment = _plan(**ALL3)
    tr.augment_seed = 4
    seen, orig = [], tr.augment_batch

    def rec(x, seed):
        out = orig(x, seed)
        seen.append((x.numpy().copy(), seed, out.cpu().numpy(), tr.last_shifts.cpu().numpy()))
        return out

    tr.augment_batch = rec
    tr.train()
    tr.valid()
    tr.test()
    assert [s for _, s, _, _ in seen] == [augment.batch_seed(4, 0, 0, i) for i in range(2)]
    for i, (x, seed, out, s) in enumerate(seen):
        want, ws = R.reference(X[4 * i:4 * i + 4], plan.coord, plan.id_at, plan.plan, seed)
        assert (x == X[4 * i:4 * i + 4]).all() and (out == want).all() and (s == ws).all() and (ws != 0).any()
