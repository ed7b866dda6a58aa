"""Worker of tests/test_parallel_two_ranks_gpu.py: ONE rank of a two-rank data-parallel job over gloo, both ranks on cuda:0.

RCCL refuses two ranks on one device; gloo does not (it stages device tensors through pinned host memory), and the product joins whatever
group is already initialised (pretrain._dist_init). `main(rank, port, out_dir, data_seed)` is the spawn target: it sets RANK / WORLD_SIZE /
LOCAL_RANK, joins the group BEFORE the first GPU call, runs every leg below with the real Engine, GradReducer and Pretrainer, and writes
`rank<r>/result.json` (scalars, SHA-256 digests, exception texts) for the parent, which only reads. Rank 0 finally computes the one-process
references (the same Engine without a hook on the global batch) against the gradients it kept on the device.

Bit-identity is recorded as the SHA-256 of a tensor's raw bytes: equal digests are torch.equal (and stricter: -0.0 differs from 0.0, NaN
payloads count), and a step's five 13 MB buffers need not travel through the file system. Leg 5 alone exchanges a tensor through a file:
each rank needs the other's gradients from before the exchange to restate it. After every leg the ranks also read each other's digests,
and where they disagree each saves the gradients, sums and parameters it kept of that leg (`rank<r>/differs_<leg>.pt`, named in the
result), so that a parity failure can be located and sized.

A leg's Python exception is recorded and the next leg runs, unless the text names the HIP runtime or a native call failed: then the rank
stops. After every leg the two ranks compare notes through small status files. The next leg runs only when both finished it, or both
raised the same error and not a time-out (gloo refusing a dtype, say): when one rank alone failed, or one raised in front of a collective
and the other waited for it in vain, their collectives no longer pair up and both stop there."""
import contextlib
import datetime
import hashlib
import io
import json
import os
import random
import time
import traceback

import numpy as np
import torch

S, D, LAYERS, FFN, HEADS, WEIGHT_SEED = 128, 256, 2, 512, 4, 51          # the _lm shapes of tests/test_grad_accum_gpu.py
B_GLOBAL, B_RANK = 8, 4
SHORT = 40                      # rank 0: lengths 20 .. 40 in the window of S -> at most 164 live rows a side, packed into one 256-row tile
LONG_MIN = S - 8                # rank 1: lengths 120 .. 128 -> at least 480 of 512 rows live, nothing to gain, dense
STEPS, LR = 3, 1e-3
PRECISIONS = ('fp32', 'bf16', 'bf16x3')
DATA_SEED = 76                  # of the even seeds 0 .. 78 the one whose smallest top-2 logit gap stays largest over the three steps (1.5e-3)
PEER_WAIT = 150.0               # seconds a rank waits for the other one's note after a leg (rank 1 waits for rank 0's references at the end)
TRAINER_S, TRAINER_N, TRAINER_VAL = 64, 24, 8


SAME_BITS = ('G', 'sums_digest', 'P', 'm', 'v')          # the digests in a leg's record that both ranks must share, in every leg that has them


def digest(t):
    a = t.detach().contiguous().cpu().view(torch.uint8).numpy()
    return hashlib.sha256(a).hexdigest()


def rank_bits_differ(mine, theirs):
    return sorted(k for k in mine if mine[k] != theirs.get(k))


def rel(a, b):
    """max|a - b| / max|b| in float64 (tests/test_grad_accum_gpu.py:_rel)."""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def global_batch(seed=DATA_SEED):
    """The global batch of 8 as CPU tensors (enc, dec, loss_mask, emask, dmask, target), ids int64: samples 0 - 3 short (rank 0), 4 - 7
    near full length (rank 1); sample 0 carries exactly 9 loss positions (tests/test_parallel_cpu.py:73)."""
    from tests.golden_util import PAD, synth_octuple_batch
    enc_s, _, lm_s, _, _, tgt_s = synth_octuple_batch(B_RANK, SHORT, seed=seed)
    enc_l, _, lm_l, _, _, tgt_l = synth_octuple_batch(B_RANK, S, seed=seed + 1, min_len=LONG_MIN)
    tail = torch.from_numpy(PAD).expand(B_RANK, S - SHORT, 8)
    enc = torch.cat([torch.cat([enc_s, tail], 1), enc_l], 0)
    tgt = torch.cat([torch.cat([tgt_s, tail], 1), tgt_l], 0)
    lm = torch.cat([torch.cat([lm_s, torch.zeros(B_RANK, S - SHORT, 8)], 1), lm_l], 0)
    dec = torch.empty_like(tgt)
    dec[:, 1:] = tgt[:, :-1]
    dec[:, 0] = torch.from_numpy(PAD + 2)                       # SOS row
    lm[0] = 0; lm[0, :9] = 1
    em, dm = (enc[:, :, 0] != int(PAD[0])).float(), (dec[:, :, 0] != int(PAD[0])).float()
    return tuple(t.contiguous() for t in (enc, dec, lm, em, dm, tgt))


def engine_args(batch, lo, hi):
    """Rows lo .. hi - 1 of a global_batch() on the device, as Engine.loss_and_grads takes them."""
    from pianobart_amd import ops
    enc, dec, lm, em, dm, tgt = (t[lo:hi].contiguous().cuda() for t in batch)
    return (ops.ids_to_i16(enc), ops.ids_to_i16(dec), ops.ids_to_i16(tgt), lm, em, dm)


def make_engine(precision, dropout=0.0):
    """A fresh model with the same seeded weights in every precision, on every rank and in the one-process reference."""
    from pianobart_amd.model import BartConfig, PianoBart, PianoBartLM
    from tests.golden_util import load_vocab, randomize_params
    e2w, w2e = load_vocab()
    cfg = BartConfig(max_position_embeddings=S, d_model=D, encoder_layers=LAYERS, decoder_layers=LAYERS, encoder_ffn_dim=FFN, decoder_ffn_dim=FFN,
                     encoder_attention_heads=HEADS, decoder_attention_heads=HEADS, dropout=dropout)
    m = PianoBartLM(PianoBart(cfg, e2w, w2e, precision=precision))
    randomize_params(m, WEIGHT_SEED)
    m = m.train().cuda()
    eng = m._get_engine()
    eng.bind(torch.device('cuda', 0))
    return m, eng


def load_parameters(m, eng, P):
    """Hand the flat f32 parameters P of another engine of the same layout to (m, eng) by the route Pretrainer.resume takes: load_state_dict
    into the modules, Engine.bind, Engine.refresh_shadow(force=True)."""
    sd = m.state_dict()
    view = {id(p): v for p, v in zip(eng.params, eng.grad_views_of(P))}
    for name, p in m.named_parameters(remove_duplicate=False):
        if id(p) in view:
            sd[name] = view[id(p)].clone()
    m.load_state_dict(sd, strict=True)
    eng.bind(torch.device('cuda', 0))
    eng.refresh_shadow(force=True)
    assert torch.equal(eng.P32, P), 'the state dict does not cover the flat parameter buffer'


def tiles_once(ranges, n_total):
    cover = np.zeros(n_total, dtype=np.int32)
    for lo, hi in ranges:
        if not 0 <= lo <= hi <= n_total:
            return False
        cover[lo:hi] += 1
    return bool((cover == 1).all())


class DeviceError(Exception):
    pass


def _names_the_device(e):
    from pianobart_amd._lib import PBError
    text = ('%s: %s' % (type(e).__name__, e)).lower()
    if isinstance(e, PBError) and ' failed (' in text:                      # a native call returned an error code
        return True
    return any(k in text for k in ('hip error', 'hiperror', 'acceleratorerror', 'illegal memory', 'hsa_status', 'device-side', 'launch failure',
                                   'unspecified launch'))


class Rank:
    def __init__(self, rank, out_dir, data_seed):
        self.rank, self.root = rank, out_dir
        self.dir = os.path.join(out_dir, 'rank%d' % rank)
        os.makedirs(self.dir, exist_ok=True)
        self.res = {'rank': rank, 'legs': {}, 'errors': {}, 'differs': {}, 'data_seed': data_seed}
        self.keep = {}                                   # device tensors rank 0 compares with the one-process references
        self.dump = {}                                   # those of the running leg: saved when the ranks' digests disagree
        self.batch = global_batch(data_seed)
        self.stopped = None

    # ---- notes between the parent and the two ranks
    def _write(self, name, obj):
        tmp = os.path.join(self.dir, name + '.tmp')
        with open(tmp, 'w') as f:
            json.dump(obj, f)
        os.replace(tmp, os.path.join(self.dir, name))

    def _peer(self, name, wait):
        path = os.path.join(self.root, 'rank%d' % (1 - self.rank), name)
        end = time.monotonic() + wait
        while not os.path.exists(path):
            if time.monotonic() > end:
                return None
            time.sleep(0.005)
        return path

    def run(self, name, fn, *args):
        if self.stopped:
            return
        self._write('progress.json', {'leg': name})
        self.dump = {}
        rec, error, fatal = None, None, False
        try:
            rec = self.res['legs'][name] = fn(*args)
            torch.cuda.synchronize()
        except Exception as e:                           # noqa: BLE001 -- recorded, reported by the parent
            error = ('%s: %s' % (type(e).__name__, e)).splitlines()[0]
            fatal = _names_the_device(e)
            self.res['errors'][name] = '%s: %s\n%s' % (type(e).__name__, e, traceback.format_exc(limit=8))
        bits = {k: rec[k] for k in SAME_BITS if k in rec} if isinstance(rec, dict) else {}
        self._write('status_%s.json' % name, {'error': error, 'bits': bits})
        if fatal:
            self.stopped = 'device error in ' + name
            return
        path = self._peer('status_%s.json' % name, PEER_WAIT)
        if path is None:
            self.stopped = 'no note from the other rank after ' + name
            return
        peer = json.load(open(path))
        if (error is None) != (peer['error'] is None):
            self.stopped = 'only one rank failed in %s: the collectives no longer pair up' % name
        elif error is not None and (error != peer['error'] or 'timed out' in error.lower() or 'timeout' in error.lower()):
            # one rank raised in front of a collective and the other waited for it in vain: what follows would pair up by chance
            self.stopped = 'the ranks failed apart in %s (the other one: %s)' % (name, peer['error'])
        elif error is None and rank_bits_differ(bits, peer['bits']) and self.dump:
            # digests say THAT the ranks differ; the tensors this rank kept say where and by how much (torch.load both files)
            file = os.path.join(self.dir, 'differs_%s.pt' % name)
            torch.save({k: [t.cpu() for t in v] if isinstance(v, list) else v.cpu() for k, v in self.dump.items()}, file)
            self.res['differs'][name] = dict(keys=rank_bits_differ(bits, peer['bits']), file=file)

    def finish(self):
        self.res['stopped'] = self.stopped
        self._write('result.json', self.res)

    # ---- legs 1 + 2: the schedule, and three optimizer steps on the gradient of the global loss
    def my_args(self):
        return engine_args(self.batch, self.rank * B_RANK, (self.rank + 1) * B_RANK)

    def leg_steps(self, precision, own_counts=False):
        from pianobart_amd.parallel import GradReducer
        m, eng = make_engine(precision)
        seed0 = int(eng._seed)
        red = GradReducer(eng, 2, mode='f32')
        seen, count_shapes = [], []
        inner = red._on_ready
        eng.grad_hook = lambda lo, hi: (seen.append((lo, hi)), inner(lo, hi))[1]
        hook = None if own_counts else (lambda c: (count_shapes.append(list(c.shape)), red.reduce_counts(c))[1])
        args = self.my_args()
        out = dict(n_total=eng.n_total, seed=str(seed0), ranges=[], count_shapes=[], last_rows=[], tiles=[], G=[], sums=[], sums_digest=[], P=[], m=[], v=[])
        keep = self.keep.setdefault('own_counts' if own_counts else precision, dict(P_before=[], G=[], sums=[]))
        self.dump = keep
        try:
            for _ in range(1 if own_counts else STEPS):
                torch.cuda.synchronize()
                keep['P_before'].append(eng.P32.clone())
                seen.clear(); count_shapes.clear()
                sums = eng.loss_and_grads(*args, train=True, count_hook=hook)
                red.all_reduce_grads()
                G = eng.G32.clone()
                sums = sums.clone()
                red.reduce_sums(sums)
                if not own_counts:
                    eng.optimizer_step(lr=LR)
                    eng.finish_updates()
                torch.cuda.synchronize()
                keep['G'].append(G); keep['sums'].append(sums)
                out['ranges'].append([list(r) for r in seen]); out['count_shapes'].append(list(count_shapes)); out['last_rows'].append(list(eng.last_rows))
                out['tiles'].append(tiles_once(seen, eng.n_total))
                out['G'].append(digest(G)); out['sums_digest'].append(digest(sums)); out['sums'].append(sums.double().cpu().tolist())
                if not own_counts:
                    out['P'].append(digest(eng.P32)); out['m'].append(digest(eng.opt_m)); out['v'].append(digest(eng.opt_v))
            keep['P_after'] = eng.P32.clone()
            out['side_stream'] = bool(eng._side)
            out['pending_after'] = len(red.pending)
        finally:
            red.close()
        return out

    # ---- leg 3: the pipelined AdamW pass behind the reducer
    def leg_pipelined(self):
        from pianobart_amd.parallel import GradReducer
        out = {}
        args = self.my_args()
        for how in ('back_to_back', 'read_every_step'):
            for pipelined in (False, True):
                m, eng = make_engine('bf16')
                eng.pipeline_updates = pipelined
                red = GradReducer(eng, 2, mode='f32')
                state = lambda: [digest(t) for t in (eng.P32, eng.opt_m, eng.opt_v, eng.Pbf)]
                rec = dict(G=[], state=[])
                try:
                    grads = []
                    for _ in range(STEPS):
                        eng.loss_and_grads(*args, train=True, count_hook=red.reduce_counts)
                        red.all_reduce_grads()
                        if how == 'back_to_back':
                            grads.append(eng.G32.clone())          # on the step's stream: nothing waits for the update on the second one
                        eng.optimizer_step(lr=LR)
                        if how == 'read_every_step':
                            eng.finish_updates()
                            torch.cuda.synchronize()
                            rec['state'].append(state())
                    eng.finish_updates()
                    torch.cuda.synchronize()
                    if how == 'back_to_back':
                        rec['G'] = [digest(g) for g in grads]
                        rec['state'].append(state())
                    rec['side_stream'] = bool(eng._side)
                finally:
                    red.close()
                out['%s/%s' % (how, 'pipelined' if pipelined else 'plain')] = rec
        return out

    # ---- leg 4: K = 2 micro-batches per rank through pretrain.run_micro_batches
    def leg_accumulated(self, precision):
        from pianobart_amd import ops, pretrain
        from pianobart_amd.parallel import GradReducer
        m, eng = make_engine(precision)
        red = GradReducer(eng, 2, mode='f32')
        calls, seen = [0], []
        exchange = red.reduce_counts
        red.reduce_counts = lambda c: (calls.__setitem__(0, calls[0] + 1), exchange(c))[1]
        inner = red._on_ready
        eng.grad_hook = lambda lo, hi: (seen.append((lo, hi)), inner(lo, hi))[1]
        lo = self.rank * B_RANK
        micro = [engine_args(self.batch, lo, lo + 2), engine_args(self.batch, lo + 2, lo + 4)]
        try:
            total = eng.mask_counts(micro[0][3])
            ops.accum_f32(total, eng.mask_counts(micro[1][3]), add=True)
            step_sums = torch.empty(24, dtype=torch.float32, device='cuda')
            sums = pretrain.run_micro_batches(eng, red, micro, total, step_sums, train=True)
            red.all_reduce_grads()
            G = eng.G32.clone()
            sums = sums.clone()
            red.reduce_sums(sums)
            torch.cuda.synchronize()
        finally:
            red.close()
        self.keep['accumulated_' + precision] = self.dump = dict(G=G, sums=sums)
        return dict(reduce_counts_calls=calls[0], tiles=tiles_once(seen, eng.n_total), ranges=[list(r) for r in seen], G=digest(G), sums_digest=digest(sums),
                    sums=sums.double().cpu().tolist(), last_rows=list(eng.last_rows))

    # ---- leg 5: the bf16 exchange, restated from both ranks' gradients before it
    def leg_bf16_exchange(self):
        from pianobart_amd.parallel import GradReducer
        m, eng = make_engine('bf16')
        red = GradReducer(eng, 2, mode='bf16')
        before = torch.zeros_like(eng.G32)
        seen = []
        inner = red._on_ready

        def hook(lo, hi):
            seen.append((lo, hi))
            before[lo:hi].copy_(eng.G32[lo:hi])          # on the announcing stream, in front of the exchange of this range
            return inner(lo, hi)

        eng.grad_hook = hook
        try:
            eng.loss_and_grads(*self.my_args(), train=True, count_hook=red.reduce_counts)
            red.all_reduce_grads()
            torch.cuda.synchronize()
        finally:
            red.close()
        tmp = os.path.join(self.dir, 'before_exchange.pt.tmp')
        torch.save(before.cpu(), tmp)
        os.replace(tmp, os.path.join(self.dir, 'before_exchange.pt'))
        path = self._peer('before_exchange.pt', PEER_WAIT)
        if path is None:
            raise RuntimeError('the other rank wrote no gradients')
        other = torch.load(path).cuda()
        g0, g1 = (before, other) if self.rank == 0 else (other, before)
        bf = lambda t: t.to(torch.bfloat16).float()
        want = torch.empty_like(before)
        for lo, hi in seen:                               # bucket by bucket (the chunks of a bucket are slices of it: the sum is elementwise)
            want[lo:hi] = bf(bf(g0[lo:hi]) + bf(g1[lo:hi]))
        return dict(equal=bool(torch.equal(want, eng.G32)), max_abs_diff=float((want - eng.G32).abs().max()), from_f32_sum=rel(eng.G32, g0 + g1),
                    tiles=tiles_once(seen, eng.n_total), G=digest(eng.G32), payloads_differ=not torch.equal(g0, g1))

    # ---- leg 6: dropout
    def leg_dropout(self):
        from pianobart_amd.parallel import GradReducer
        m, eng = make_engine('bf16', dropout=0.1)
        seed0 = int(eng._seed)
        red = GradReducer(eng, 2, mode='f32')
        out = dict(seed=str(seed0), p_drop=eng.p_drop, P=[], sums=[])
        args = self.my_args()
        try:
            for _ in range(2):
                sums = eng.loss_and_grads(*args, train=True, count_hook=red.reduce_counts)
                red.all_reduce_grads()
                sums = sums.clone()
                red.reduce_sums(sums)
                eng.optimizer_step(lr=LR)
                eng.finish_updates()
                torch.cuda.synchronize()
                out['P'].append(digest(eng.P32)); out['sums'].append(sums.double().cpu().tolist())
        finally:
            red.close()
        return out

    # ---- leg 7: an id at its table's limit on rank 1 only, module route
    def leg_bad_id(self):
        from pianobart_amd.parallel import GradReducer
        from tests.golden_util import N_TOK
        m, eng = make_engine('bf16')
        m.train()
        red = GradReducer(eng, 2, mode='f32')
        lo = self.rank * B_RANK
        enc, dec, lm, em, dm, tgt = (t[lo:lo + B_RANK].contiguous().cuda() for t in self.batch)
        bad = enc.clone()
        if self.rank == 1:
            bad[1, 5, 3] = N_TOK[3]                       # the first id outside head 3's table
        out = dict(raised=None, bad_here=bool((bad != enc).any()))
        try:
            try:
                m(bad, dec, em, dm)
            except IndexError as e:
                out['raised'] = 'IndexError: %s' % e
            y = m(enc, dec, em, dm)                       # a clean step right behind it
            loss = 0
            for i in range(8):
                ce = torch.nn.functional.cross_entropy(y[i].permute(0, 2, 1), tgt[..., i], reduction='none')
                loss = loss + (ce * lm[..., i]).sum() / lm[..., i].sum()
            m.zero_grad()
            loss.backward()
            red.all_reduce_grads()
            torch.cuda.synchronize()
            out.update(G=digest(eng.G32), finite=bool(torch.isfinite(eng.G32).all()), nonzero=bool(eng.G32.abs().max() > 0), loss=float(loss))
        finally:
            red.close()
        return out

    # ---- leg 8: the trainer
    def leg_trainer(self):
        from pianobart_amd import pretrain
        from pianobart_amd.model import BartConfig, PianoBart
        from tests.golden_util import load_vocab, synth_octuple_batch
        e2w, w2e = load_vocab()
        work = os.path.join(self.dir, 'cwd')
        os.makedirs(work, exist_ok=True)
        os.chdir(work)                                    # result/pretrain/<name> is relative to the working directory
        random.seed(100 + self.rank); np.random.seed(200 + self.rank)      # the corruption draws; rank 0's sampler seed becomes everyone's
        X = synth_octuple_batch(TRAINER_N + TRAINER_VAL, TRAINER_S, seed=40)[5].numpy().astype(np.int16)
        train_loader, valid_loader = pretrain.make_loaders(X[:TRAINER_N], X[TRAINER_N:], B_GLOBAL, 0, pad_bar=int(e2w['Bar']['Bar <PAD>']))
        cfg = BartConfig(max_position_embeddings=TRAINER_S, d_model=D, encoder_layers=LAYERS, decoder_layers=LAYERS, encoder_ffn_dim=FFN, decoder_ffn_dim=FFN,
                         encoder_attention_heads=HEADS, decoder_attention_heads=HEADS)
        pb = PianoBart(cfg, e2w, w2e)                     # unseeded, like pretrain.pretrain(): every process draws its own initial weights
        built = digest(torch.cat([p.detach().reshape(-1) for p in pb.parameters()]))
        tr = pretrain.Pretrainer(pb, train_loader, valid_loader, LR, B_GLOBAL, TRAINER_S, 0.15, False, [0])
        out = dict(P_built=built, world=tr.world, trainer_rank=tr.rank, reducer=type(tr.reducer).__name__, mode=getattr(tr.reducer, 'mode', None),
                   pipeline_updates=bool(tr.engine.pipeline_updates), sampler=type(train_loader.sampler).__name__, sampler_seed=int(train_loader.sampler.seed),
                   per_rank_batch=train_loader.batch_size, steps_per_epoch=len(train_loader), P_init=digest(tr.engine.P32), step_seed=str(tr._step_seed))
        train_loader.sampler.set_epoch(0)
        out['indices'] = [int(i) for i in train_loader.sampler]
        buf = io.StringIO()
        try:
            with contextlib.redirect_stdout(buf):
                loss, accs = tr.train()
            tr.engine.finish_updates()
            torch.cuda.synchronize()
            out.update(loss=loss, accs=list(accs), lines=[l for l in buf.getvalue().splitlines() if l.startswith(('Loss:', 'Acc:'))],
                       P=digest(tr.engine.P32), steps=tr.engine.step_count, finite=bool(torch.isfinite(tr.engine.P32).all()))
            # the tail of pretrain.pretrain(): the rank comes from the environment, and both gates (checkpoint, log) are _RunLog's
            run = pretrain._RunLog('two_ranks', pretrain._dist_env()[0] == 0)
            run.save(tr, 0, 0.0, accs, loss, loss, True)
            run.write('Epoch 1: train_loss={}, train_acc={}\n'.format(loss, accs))
            out['files'] = sorted(os.path.relpath(os.path.join(d, f), work) for d, _, fs in os.walk(work) for f in fs)
        finally:
            tr.reducer.close()
        return out

    # ---- rank 0: the one-process references
    def leg_references(self):
        batch = self.batch
        args = engine_args(batch, 0, B_GLOBAL)
        ref = {p: make_engine(p) for p in PRECISIONS}
        out = {'steps': {}, 'top2_gap': [], 'last_rows': {}}

        def grads(p, P):
            m, eng = ref[p]
            load_parameters(m, eng, P)
            sums = eng.loss_and_grads(*args, train=True)
            torch.cuda.synchronize()
            out['last_rows'][p] = list(eng.last_rows)
            return eng.G32.clone(), sums.clone()

        def sums_record(got, want):
            return dict(counts_equal=bool(torch.equal(got[8:16], want[8:16])), hits_equal=bool(torch.equal(got[16:24], want[16:24])),
                        loss_rel=rel(got[0:8], want[0:8]), hits=got[16:24].tolist(), hits_ref=want[16:24].tolist())

        first = {}
        for p in PRECISIONS:
            k, rows = self.keep[p], []
            for s in range(STEPS):
                G, sums = grads(p, k['P_before'][s])
                r = dict(err=rel(k['G'][s], G), **sums_record(k['sums'][s], sums))
                if p != 'fp32':
                    G32, sums32 = grads('fp32', k['P_before'][s])
                    r['own'] = rel(G, G32)                       # this precision's own distance from fp32: same batch, same parameters, same run
                else:
                    r['top2_gap'] = self._top2_gap(ref['fp32'][0], batch)
                if s == 0:
                    first[p] = (G, sums, r.get('own'))
                rows.append(r)
            out['steps'][p] = rows
        out['own_counts'] = rel(self.keep['own_counts']['G'][0], first['fp32'][0])
        for p in ('fp32', 'bf16'):
            G, sums, own = first[p]
            k = self.keep['accumulated_' + p]
            out['accumulated_' + p] = dict(err=rel(k['G'], G), own=own, **sums_record(k['sums'], sums))
        return out

    @staticmethod
    def _top2_gap(m, batch):
        """Smallest distance between the two largest logits of a head at a loss position, over the global batch (eval forward, dropout 0)."""
        enc, dec, lm, em, dm, tgt = (t.cuda() for t in batch)
        m.eval()
        try:
            with torch.no_grad():
                y = m(enc, dec, em, dm)
        finally:
            m.train()
        gap = float('inf')
        for i in range(8):
            top = y[i].float().topk(2, dim=-1).values
            g = (top[..., 0] - top[..., 1])[lm[..., i] > 0]
            gap = min(gap, float(g.min()))
        return gap


def main(rank, port, out_dir, data_seed=DATA_SEED):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE='2', LOCAL_RANK='0')
    os.environ.pop('PB_DP_GRADS', None)
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=2, timeout=datetime.timedelta(seconds=90))       # before any GPU call
    me = Rank(rank, out_dir, data_seed)
    try:
        torch.cuda.set_device(0)
        for p in PRECISIONS:
            me.run('steps_' + p, me.leg_steps, p)
        me.run('own_counts', me.leg_steps, 'fp32', True)
        me.run('pipelined', me.leg_pipelined)
        for p in ('fp32', 'bf16'):
            me.run('accumulated_' + p, me.leg_accumulated, p)
        me.run('bf16_exchange', me.leg_bf16_exchange)
        me.run('dropout', me.leg_dropout)
        me.run('bad_id', me.leg_bad_id)
        me.run('trainer', me.leg_trainer)
        me.run('references', me.leg_references if rank == 0 else (lambda: None))
    finally:
        me.finish()
        dist.destroy_process_group()
