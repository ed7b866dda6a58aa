"""GPU, world size 2 over gloo, both ranks on ONE device: the data-parallel step with two real engines that do exchange bytes.

tests/test_parallel_cpu.py runs gloo at world 2 with a flat tensor for an engine; tests/test_parallel_gpu.py runs the real Engine at
world 1, where every collective is the identity. Here two fresh processes (tests/dp_two_ranks.py) join a gloo group before their first GPU
call -- RCCL refuses two ranks on one device, gloo does not, and the product joins the group it finds (pretrain._dist_init) -- and run
the product step on cuda:0: Engine.loss_and_grads with the count exchange, GradReducer's bucket exchange from both streams, optimizer_step,
pretrain.run_micro_batches, PianoBartLM's training forward and the Pretrainer. One module-scoped fixture starts them once and waits with
a time limit of its own; the tests only read what the ranks recorded. Bit-identity is compared through SHA-256 digests of the raw bytes;
where the ranks' digests disagree, each rank saves the tensors it kept of that leg and the failing assertion names the files.

Model: d = 256, 2 + 2 layers, 4 heads, ffn 512, S = 128 (the _lm shapes of tests/test_grad_accum_gpu.py), dropout 0 unless a leg says
otherwise. Global batch of 8: rank 0 steps 4 sequences of 20 .. 40 rows (packed: 256 of 512 rows a side), rank 1 steps 4 of 120 .. 128 rows
(dense); sample 0 carries 9 loss positions (tests/test_parallel_cpu.py:73), so the ranks' mask counts differ widely in every head.

Bounds and where they come from (max|dG| / max|G| against the SAME Engine without a hook stepping the global batch of 8 in one process,
loaded before every step with the parameters the two-rank run held, so that gradient is compared with gradient at equal parameters):
  * fp32: 1e-5, the bound of tests/test_parallel_cpu.py:92 and of the split batch in tests/test_grad_accum_gpu.py.
  * bf16, bf16x3: at most 2x the distance between that precision's and fp32's one-process gradient of the same batch at the same
    parameters, measured in the same run (tests/test_grad_accum_gpu.py's rule: the split adds no more than the precision's own rounding).
  * the 24 sums: mask counts exact; loss sums 1e-5 relative in every precision; correct-counts exact in fp32, given that the
    reference's smallest top-2 logit gap at a loss position exceeds 1e-3 (asserted; the data seed was picked for it). The accumulated
    step is held to the same bounds: the forward works row by row, so micro-batches of 2 change the order of the sums and no more.
  * teeth: the same two-rank step with count_hook=None (every rank normalises by its own counts) must miss the fp32 bound by 100x.
  * rank parity, pipelined against plain update, bf16 exchange against bf(bf(g0) + bf(g1)): bit for bit.

Measured on an MI355X (every run prints them again with -s); max|dG| / max|G| of steps 1, 2, 3:
  * fp32 4.2e-7, 3.9e-7, 3.7e-7 (bound 1e-5; 2.7e-7 .. 4.5e-7 over three runs, the f32 atomics of the embedding path vary); loss sums within 1.8e-7 (bound 1e-5); correct-counts equal; smallest top-2 gap 1.50e-3, 1.49e-3, 1.79e-3.
  * bf16 1.6e-3, 5.2e-7, 1.7e-7 against 2 x (2.4e-2, 1.4e-2, 9.6e-3); bf16x3 7.4e-6, 5.2e-6, 4.2e-6 against 2 x (3.6e-5, 2.3e-5, 1.2e-5);
    loss sums within 8.9e-8 in both.
  * own counts (count_hook=None): 1.4e+0.
  * accumulated 2 + 2 per rank: fp32 3.0e-7 .. 3.6e-7; bf16 1.6e-3 (bound 4.8e-2); loss sums within 7.7e-8 in both (bound 1e-5).
  * bf16 exchange: equal to bf(bf(g0) + bf(g1)) on both ranks, 3.7e-3 of max|G| from the f32 sum. gloo moves bf16 device tensors through
    all_to_all_single and all_gather_into_tensor here, so the leg runs.
  * last_rows (Te, Td, T, Ts): rank 0 (256, 256, 512, 256) in bf16 and bf16x3, rank 1 (512, 512, 512, 512); the one-process reference
    (768, 768, 1024, 256); fp32 never packs. The second stream stood on both ranks, 8 ranges per step, the fixture takes 9 - 14 s.
  * the trainer leg found ranks that started from different weights: every process seeds torch's default generator by itself and the
    Pretrainer never made them equal. It now broadcasts rank 0's parameters; the leg asserts both halves.
    The worker ends the epoch as pretrain() does, through _RunLog.save and _RunLog.write with the rank of the environment, so the gates
    that keep rank 1 from writing a checkpoint or a log are the product's.

Teeth, checked once by hand on scratch copies of parallel.py (never committed): with reduce_counts a no-op the three against-one-process
tests and the two accumulation tests fail and every rank-parity test passes; with an f32 _on_ready that skips the last announced range
the rank-parity tests fail in every precision (and with them 10 of the others)."""
import json
import os
import time

import numpy as np
import pytest
import torch

from tests import dp_two_ranks as W

pytestmark = pytest.mark.gpu
PRECISIONS = W.PRECISIONS
WAIT = 240.0


def _last_leg(out, rank):
    try:
        return json.load(open(os.path.join(str(out), 'rank%d' % rank, 'progress.json')))['leg']
    except (OSError, ValueError):
        return 'none (it never reported)'


@pytest.fixture(scope='module')
def ranks(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')                               # before any child is started
    import torch.multiprocessing as mp
    out = tmp_path_factory.mktemp('two_ranks')
    ctx = mp.get_context('spawn')
    port = 31000 + (os.getpid() % 2000)
    procs = [ctx.Process(target=W.main, args=(r, port, str(out), W.DATA_SEED)) for r in range(2)]
    t0 = time.monotonic()
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=max(0.0, t0 + WAIT - time.monotonic()))
    late = [r for r, p in enumerate(procs) if p.is_alive()]
    if late:
        for p in procs:
            p.terminate()
        for p in procs:
            p.join(timeout=30)
        pytest.fail('ranks %s still ran after %d s; last leg reported: rank 0 %s, rank 1 %s'
                    % (late, WAIT, _last_leg(out, 0), _last_leg(out, 1)))
    res = []
    for r, p in enumerate(procs):
        path = os.path.join(str(out), 'rank%d' % r, 'result.json')
        assert os.path.exists(path), 'rank %d left no result (exit code %s, last leg %s)' % (r, p.exitcode, _last_leg(out, r))
        res.append(json.load(open(path)))
        assert p.exitcode == 0, 'rank %d exit code %s; errors %s' % (r, p.exitcode, res[-1]['errors'])
    print('\ntwo ranks on one device: %.1f s from the first spawn to the last exit' % (time.monotonic() - t0))
    return res


def _leg(ranks, name, only=None):
    """The record of leg `name` of both ranks (or of one); fails with the recorded exception text when the leg did not finish."""
    got = []
    for r in ((0, 1) if only is None else (only,)):
        res = ranks[r]
        assert name not in res['errors'], 'rank %d, leg %s raised:\n%s' % (r, name, res['errors'][name])
        assert name in res['legs'], 'rank %d never ran leg %s (%s)' % (r, name, res['stopped'])
        got.append(res['legs'][name])
    return got if only is None else got[0]


def _saved(ranks, name):
    """Where the ranks saved the tensors of a leg whose digests disagree (torch.load both files to see where and by how much)."""
    return [res['differs'].get(name) for res in ranks]


def test_every_leg_ran_on_both_ranks(ranks):
    for r in (0, 1):
        assert ranks[r]['stopped'] is None and not ranks[r]['errors'], (r, ranks[r]['stopped'], ranks[r]['errors'])


# ---------------------------------------------------------------------------------------------------- 1. schedule
@pytest.mark.parametrize('precision', PRECISIONS)
def test_both_ranks_announce_the_same_exchange(ranks, precision):
    a, b = _leg(ranks, 'steps_' + precision)
    print('\n%s: last_rows (Te, Td, T, Ts) rank 0 %s, rank 1 %s; second stream %s / %s; %d ranges per step'
          % (precision, a['last_rows'][0], b['last_rows'][0], a['side_stream'], b['side_stream'], len(a['ranges'][0])))
    T = W.B_RANK * W.S
    if precision != 'fp32':                                 # the exact-f32 instantiation never packs
        assert all(rows[0] < T and rows[1] < T for rows in a['last_rows']), a['last_rows']           # rank 0 packs its rows ...
    assert all(rows[0] == T and rows[1] == T for rows in b['last_rows']), b['last_rows']             # ... rank 1 stays dense
    assert a['n_total'] == b['n_total']
    for s in range(W.STEPS):
        assert a['ranges'][s] == b['ranges'][s] and len(a['ranges'][s]) > 4, s      # the collectives pair up by issue order
        assert a['ranges'][s] == a['ranges'][0]
        assert a['tiles'][s] and b['tiles'][s]                                      # [0, n_total) exactly once
        assert a['count_shapes'][s] == b['count_shapes'][s] == [[8]]                # one exchange of the 8 mask counts
    assert a['pending_after'] == b['pending_after'] == 0


# ---------------------------------------------------------------------------------------------------- 2. gradient of the global loss
@pytest.mark.parametrize('precision', PRECISIONS)
def test_ranks_hold_identical_bits_after_every_step(ranks, precision):
    a, b = _leg(ranks, 'steps_' + precision)
    for key in W.SAME_BITS:
        assert len(a[key]) == W.STEPS and a[key] == b[key], (precision, key, _saved(ranks, 'steps_' + precision))
    assert len(set(a['P'])) == W.STEPS and len(set(a['G'])) == W.STEPS              # the steps did move the parameters


def _sums_ok(r):
    assert r['counts_equal']
    assert r['loss_rel'] <= 1e-5, r['loss_rel']


@pytest.mark.parametrize('precision', PRECISIONS)
def test_two_rank_gradient_is_the_one_process_gradient_of_the_global_batch(ranks, precision):
    ref = _leg(ranks, 'references', only=0)
    print('\none-process reference, last_rows per precision: %s' % ref['last_rows'])
    for s, r in enumerate(ref['steps'][precision]):
        bound = 1e-5 if precision == 'fp32' else 2 * r['own']
        print('%s step %d: max|dG| / max|G| = %.3e (bound %.3e); loss sums rel %.3e; counts equal %s; correct-counts %s / reference %s%s'
              % (precision, s + 1, r['err'], bound, r['loss_rel'], r['counts_equal'], r['hits'], r['hits_ref'],
                 '; smallest top-2 logit gap %.3e' % r['top2_gap'] if 'top2_gap' in r else ''))
    for s, r in enumerate(ref['steps'][precision]):
        bound = 1e-5 if precision == 'fp32' else 2 * r['own']
        assert r['err'] <= bound, (precision, s, r['err'], bound)
        _sums_ok(r)
        if precision == 'fp32':
            assert r['top2_gap'] > 1e-3, 'the data seed no longer keeps the top-2 logits apart: %r' % r['top2_gap']
            assert r['hits_equal'], (r['hits'], r['hits_ref'])


def test_own_counts_miss_the_bound_by_two_orders(ranks):
    """Teeth: count_hook=None, i.e. the step without the 8-float exchange (a mean of per-rank means)."""
    a, b = _leg(ranks, 'own_counts')
    assert a['G'] == b['G']                                  # the exchange itself still works: the loss scale is what is wrong
    miss = _leg(ranks, 'references', only=0)['own_counts']
    print('\nown counts (count_hook=None), fp32: max|dG| / max|G| = %.3e (must be >= 1e-3)' % miss)
    assert miss >= 100 * 1e-5


# ---------------------------------------------------------------------------------------------------- 3. pipelined update
def test_pipelined_update_behind_the_reducer_takes_the_same_steps(ranks):
    a, b = _leg(ranks, 'pipelined')
    print('\npipelined update: second stream %s / %s' % (a['back_to_back/pipelined']['side_stream'], b['back_to_back/pipelined']['side_stream']))
    for how in ('back_to_back', 'read_every_step'):
        plain, piped = a[how + '/plain'], a[how + '/pipelined']
        assert len(plain['state']) == (1 if how == 'back_to_back' else W.STEPS)
        assert plain['state'] == piped['state'], how         # P32, opt_m, opt_v, Pbf: bit for bit between the two settings ...
        assert plain['G'] == piped['G'], how                 # ... and so is every step's reduced gradient (steps 2, 3: of the updated parameters)
        for key in (how + '/plain', how + '/pipelined'):
            assert a[key]['state'] == b[key]['state'] and a[key]['G'] == b[key]['G'], key             # ... and across the ranks
    assert a['back_to_back/plain']['state'][0] == a['read_every_step/plain']['state'][-1]
    assert len(set(a['back_to_back/plain']['G'])) == W.STEPS


# ---------------------------------------------------------------------------------------------------- 4. accumulation
@pytest.mark.parametrize('precision', ['fp32', 'bf16'])
def test_accumulated_micro_batches_under_the_reducer(ranks, precision):
    a, b = _leg(ranks, 'accumulated_' + precision)
    assert a['G'] == b['G'] and a['sums_digest'] == b['sums_digest'], _saved(ranks, 'accumulated_' + precision)
    assert a['reduce_counts_calls'] == b['reduce_counts_calls'] == 1                # `total`, once per optimizer step
    assert a['tiles'] and b['tiles'] and a['ranges'] == b['ranges']
    assert a['ranges'] == _leg(ranks, 'steps_' + precision, only=0)['ranges'][0]    # the schedule of the step without accumulation
    r = _leg(ranks, 'references', only=0)['accumulated_' + precision]
    bound = 1e-5 if precision == 'fp32' else 2 * r['own']
    print('\naccumulated 2 + 2 per rank, %s: max|dG| / max|G| = %.3e (bound %.3e); loss sums rel %.3e (bound 1e-5); last micro-batch rows %s / %s'
          % (precision, r['err'], bound, r['loss_rel'], a['last_rows'], b['last_rows']))
    assert r['err'] <= bound
    _sums_ok(r)
    if precision == 'fp32':
        assert r['hits_equal']


# ---------------------------------------------------------------------------------------------------- 5. bf16 exchange
def test_bf16_exchange_is_one_rounding_in_and_one_out(ranks):
    a, b = _leg(ranks, 'bf16_exchange')
    print('\nbf16 exchange: max |d| from bf(bf(g0) + bf(g1)) %.3e / %.3e; %.3e of max|G| from the f32 sum' % (a['max_abs_diff'], b['max_abs_diff'], a['from_f32_sum']))
    assert a['payloads_differ'] and a['tiles'] and b['tiles']
    assert a['equal'] and b['equal']
    assert a['G'] == b['G']
    assert a['from_f32_sum'] < 8e-3                           # two bf16 roundings (tests/test_parallel_cpu.py:52)


# ---------------------------------------------------------------------------------------------------- 6. dropout
def test_dropout_streams_differ_and_parameters_do_not(ranks):
    a, b = _leg(ranks, 'dropout')
    assert a['p_drop'] == b['p_drop'] == 0.1
    assert a['seed'] != b['seed']                             # Engine._seed is keyed by RANK
    assert a['P'] == b['P'] and len(set(a['P'])) == 2
    assert np.isfinite(np.array(a['sums'] + b['sums'])).all()
    assert a['sums'] == b['sums']


# ---------------------------------------------------------------------------------------------------- 7. a bad id on one rank
def test_bad_id_on_one_rank_raises_on_both(ranks):
    a, b = _leg(ranks, 'bad_id')
    assert not a['bad_here'] and b['bad_here']
    for r in (a, b):
        assert r['raised'] is not None and r['raised'].startswith('IndexError: index out of range in self'), r['raised']
        assert r['finite'] and r['nonzero']
    assert a['G'] == b['G']                                   # the clean step behind it pairs up again


# ---------------------------------------------------------------------------------------------------- 8. the trainer
def test_pretrainer_at_world_size_two(ranks):
    from pianobart_amd.data import BalancedDistributedSampler, sequence_lengths
    from tests.golden_util import synth_octuple_batch
    a, b = _leg(ranks, 'trainer')
    for r, t in enumerate((a, b)):
        assert (t['world'], t['trainer_rank'], t['reducer'], t['mode'], t['pipeline_updates']) == (2, r, 'GradReducer', 'f32', True)
        assert t['sampler'] == 'BalancedDistributedSampler' and t['per_rank_batch'] == W.B_RANK and t['steps_per_epoch'] == 3 and t['steps'] == 3
        assert len(t['indices']) == W.TRAINER_N // 2 and t['finite']
    assert a['sampler_seed'] == b['sampler_seed']             # rank 0's draw, broadcast
    assert a['step_seed'] != b['step_seed']                   # the corruption stream is keyed by the rank
    assert not set(a['indices']) & set(b['indices'])
    X = synth_octuple_batch(W.TRAINER_N + W.TRAINER_VAL, W.TRAINER_S, seed=40)[5].numpy()[:W.TRAINER_N]
    one = list(BalancedDistributedSampler(sequence_lengths(X, 256), 1, 0, W.B_GLOBAL, shuffle=True, seed=a['sampler_seed']))
    g = torch.Generator()
    g.manual_seed(a['sampler_seed'])
    assert sorted(one) == list(range(W.TRAINER_N)) and set(one[:8]) == set(torch.randperm(W.TRAINER_N, generator=g)[:8].tolist())
    for s in range(3):                                        # step s: the two shares are the single-process global batch of the same seed
        mine = a['indices'][4 * s:4 * s + 4] + b['indices'][4 * s:4 * s + 4]
        assert sorted(mine) == sorted(one[8 * s:8 * s + 8]), s
    assert a['P_built'] != b['P_built']                       # two processes, two unseeded initialisations ...
    assert a['P_init'] == b['P_init']                         # ... and one set of parameters once the trainer stands: rank 0's
    assert a['P'] == b['P'] and a['P'] != a['P_init']
    assert a['loss'] == b['loss'] and a['accs'] == b['accs'] and np.isfinite(a['loss'])
    assert a['lines'] == b['lines'] and len(a['lines']) == 6  # the Loss / Acc lines of the three steps
    print('\ntrainer: epoch loss %s, %s' % (a['loss'], a['lines'][0]))
    assert sorted(a['files']) == sorted(os.path.join('result', 'pretrain', 'two_ranks', f) for f in ('log', 'model.ckpt', 'model_best.ckpt'))
    assert b['files'] == []                                   # rank 1 writes neither checkpoint nor log
