"""LoRA fine-tuning: trainable rank-r adapters on the attention projections of a frozen backbone (DESIGN.md 5 "LoRA").

A chosen projection y = x W^T + b gains the term s (x A^T) B^T with A (r, K), B (N, r), s = alpha / r. The backbone's flat buffers are
left alone: every adapter lives in ONE flat f32 buffer of this module with a gradient buffer of the same layout beside it, the engine's
forward, backward and optimizer step call into LoraState at the three places where a q / k / v projection is made (Engine.forward_hidden)
and where its cotangent is final (Engine.backward), and the arithmetic is the four kernels of csrc/pb_lora.hip (ops.lora_*).

  cfg = lora.LoraConfig(rank=8, alpha=16, targets=('q', 'v', 'cq', 'cv'))
  eng.attach_lora(cfg, seed=0)            # freezes the backbone; the LM heads keep training unless train_heads=False
  ... eng.loss_and_grads(...); eng.optimizer_step(lr) ...
  lora.save('a.lora.pt', model)           # a few MB: A / B per site, the heads, the moments; never a backbone tensor
  eng.merge_lora()                        # W += s B A in the f32 masters: a plain model again (generation, scoring, model_merge ..)

python -m pianobart_amd.lora --ckpt base.ckpt --lora a.lora.pt --output merged.ckpt folds an adapter file into a whole checkpoint.
"""
import argparse
import math
import os

import torch

from . import ops
from ._lib import PBError

TARGETS = ('q', 'k', 'v', 'cq', 'ck', 'cv')         # self-attention q / k / v (encoder and decoder layers), the decoder's cross-attention q / k / v
RANK_MIN, RANK_MAX = 4, 64
FORMAT = 'pianobart_amd.lora/1'


class LoraConfig:
    """rank: r, a multiple of 4 in 4 .. 64 (and <= d_model); alpha: the scale numerator, s = alpha / rank; targets: names out of TARGETS."""

    def __init__(self, rank=8, alpha=16, targets=('q', 'v', 'cq', 'cv')):
        self.rank, self.alpha = rank, alpha
        self.targets = (targets,) if isinstance(targets, str) else tuple(targets)

    @property
    def scale(self):
        return float(self.alpha) / float(self.rank)

    def check(self, d_model=None):
        r = self.rank
        if not isinstance(r, int) or isinstance(r, bool) or r < RANK_MIN or r > RANK_MAX or r % 4:
            raise PBError('LoRA rank must be a multiple of 4 in %d .. %d (got %r)' % (RANK_MIN, RANK_MAX, r))
        if d_model is not None and r > d_model:
            raise PBError('LoRA rank %d exceeds d_model %d' % (r, d_model))
        try:
            ok = math.isfinite(float(self.alpha))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise PBError('LoRA alpha must be a finite number (got %r)' % (self.alpha,))
        if not self.targets:
            raise PBError('LoRA targets are empty: name at least one of %s' % ', '.join(TARGETS))
        for t in self.targets:
            if t not in TARGETS:
                raise PBError('unknown LoRA target %r: the targets are %s' % (t, ', '.join(TARGETS)))
        if len(set(self.targets)) != len(self.targets):
            raise PBError('LoRA targets name %s twice' % sorted(t for t in set(self.targets) if self.targets.count(t) > 1))
        return self

    def to_dict(self):
        return dict(rank=int(self.rank), alpha=float(self.alpha), targets=list(self.targets))

    def __repr__(self):
        return 'LoraConfig(rank=%r, alpha=%r, targets=%r)' % (self.rank, self.alpha, self.targets)


def parse_targets(text):
    """'q,v,cq,cv' -> ('q', 'v', 'cq', 'cv'); PBError names an unknown one."""
    names = tuple(t.strip() for t in str(text).split(',') if t.strip())
    LoraConfig(rank=RANK_MIN, targets=names).check()
    return names


def add_arguments(parser):
    """finetune_generation's adapter flags (off by default)."""
    parser.add_argument('--lora_rank', type=int, default=0, metavar='R', help='train rank-R LoRA adapters on a frozen backbone instead of the whole model '
                        '(a multiple of 4 in 4 .. 64; 0 = off); the checkpoint becomes model.lora.pt (not in the reference)')
    parser.add_argument('--lora_alpha', type=float, default=None, metavar='A', help='the adapter scale is A / R (default: 2 R)')
    parser.add_argument('--lora_targets', type=str, default='q,v,cq,cv', help='projections that get an adapter, out of ' + ','.join(TARGETS))
    parser.add_argument('--lora_seed', type=int, default=0, metavar='N', help='seed of the adapters\' initialisation')
    parser.add_argument('--lora_freeze_heads', action='store_true', help='freeze the LM heads too (default: they train beside the adapters)')


def from_args(args):
    """The LoraConfig of the flags, or None when --lora_rank is 0. Everything that can be refused without a device is refused here."""
    rank = int(getattr(args, 'lora_rank', 0) or 0)
    given = [f for f in ('lora_alpha',) if getattr(args, f, None) is not None]
    if getattr(args, 'lora_freeze_heads', False):
        given.append('lora_freeze_heads')
    if rank == 0:
        if given:
            raise PBError('--%s needs --lora_rank' % given[0])
        return None
    cfg = LoraConfig(rank=rank, alpha=args.lora_alpha if args.lora_alpha is not None else 2 * rank, targets=parse_targets(args.lora_targets)).check()
    if int(getattr(args, 'accum_steps', 1)) > 1:
        raise PBError('--lora_rank does not combine with --accum_steps %d: gradient accumulation sums the flat backbone gradient' % args.accum_steps)
    if int(os.environ.get('WORLD_SIZE', 1)) > 1:
        raise PBError('--lora_rank does not combine with a multi-rank launch (WORLD_SIZE = %s): the reducer buckets the flat backbone gradient'
                      % os.environ.get('WORLD_SIZE'))
    return cfg


class _Site:
    """One adapted projection: where its A / B and their gradients sit in the flat buffers, which module it belongs to and which slot rows it merges into."""
    __slots__ = ('key', 'module', 'slot', 'row', 'K', 'N', 'off_a', 'off_b', 'A', 'B', 'gA', 'gB', 't')


def _site_list(eng, targets):
    """[(hook group, column offset of the site's slice in the group's output buffer, _Site)] in a fixed order: encoder layers, then decoder layers."""
    d, pb = eng.d, eng.pb
    out = []

    def add(group, col, key, module, slot, row):
        s = _Site()
        s.key, s.module, s.slot, s.row, s.K, s.N, s.t = key, module, slot, row, d, d, None
        out.append((group, col, s))

    for side, stack, n in (('enc', pb.bart.encoder, eng.NE), ('dec', pb.bart.decoder, eng.ND)):
        for l in range(n):
            L, p = stack.layers[l], '%s.%d.' % (side, l)
            for i, (t, mod) in enumerate((('q', L.self_attn.q_proj), ('k', L.self_attn.k_proj), ('v', L.self_attn.v_proj))):
                if t in targets:
                    add(p + 'qkv', i * d, p + t, mod, p + 'wqkv', i * d)
            if side == 'dec':
                ca = L.encoder_attn
                if 'cq' in targets:
                    add(p + 'cq', 0, p + 'cq', ca.q_proj, p + 'wq_c', 0)
                for i, (t, mod) in enumerate((('ck', ca.k_proj), ('cv', ca.v_proj))):
                    if t in targets:
                        add(p + 'ckv', l * 2 * d + i * d, p + t, mod, 'dec.wkv_all', l * 2 * d + i * d)
    return out


class LoraState:
    """What Engine.attach_lora builds: the flat adapter buffers, the sites, and the forward / backward / step / merge calls the engine makes."""

    def __init__(self, eng, cfg, seed, train_heads):
        self.cfg, self.r, self.s = cfg, int(cfg.rank), cfg.scale
        self.train_heads = bool(train_heads) and eng.mlm is not None
        entries = _site_list(eng, cfg.targets)
        if not entries:
            raise PBError('LoRA targets %s name no projection of this model (%d encoder, %d decoder layers)' % (list(cfg.targets), eng.NE, eng.ND))
        self.sites, self.groups, cur = [], {}, 0
        for group, col, s in entries:
            s.off_a, s.off_b = cur, cur + self.r * s.K
            cur = s.off_b + s.N * self.r
            self.sites.append(s)
            self.groups.setdefault(group, []).append((s, col))
        self.n = cur
        dev = eng.device
        self.P = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.G = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.m = self.v = None                       # adapter moments, allocated by the first step
        self.head_m = self.head_v = None             # {slot name: moment} of head.w / head.b
        gen = torch.Generator().manual_seed(int(seed))
        for s in self.sites:
            s.A, s.B = self.P[s.off_a:s.off_b].view(self.r, s.K), self.P[s.off_b:s.off_b + s.N * self.r].view(s.N, self.r)
            s.gA, s.gB = self.G[s.off_a:s.off_b].view(self.r, s.K), self.G[s.off_b:s.off_b + s.N * self.r].view(s.N, self.r)
            bound = 1.0 / math.sqrt(s.K)
            s.A.copy_(((torch.rand(self.r, s.K, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound).to(dev))
        self._dT = self._ws = None
        self._head_table = None

    # ---- scratch -----------------------------------------------------------------------------------------------------------------------
    def _rows(self, eng):
        ws = eng._cur_ws
        return int(ws.get('_base', ws)['T'])

    def _t_of(self, eng, site):
        """t = x A^T of the site's last forward, (rows of the workspace, r) f32: kept for the backward (dB = s dY^T t)."""
        T = self._rows(eng)
        if site.t is None or site.t.shape[0] < T:
            site.t = torch.empty(T, self.r, dtype=torch.float32, device=eng.device)
        return site.t

    def _scratch(self, eng, M, C):
        T = self._rows(eng)
        if self._dT is None or self._dT.shape[0] < T:
            self._dT = torch.empty(T, self.r, dtype=torch.float32, device=eng.device)
        need = int(ops.LIB.query('pb_lora_wgrad_ws_floats', int(M), self.r, int(C)))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(4, need), dtype=torch.float32, device=eng.device)
        return self._dT, self._ws

    # ---- the engine's hooks ------------------------------------------------------------------------------------------------------------
    def forward(self, eng, group, x, y, M):
        """Behind the base GEMM y = x W^T + b of `group`, on its stream and over its M rows: y[:, slice] += s (x A^T) B^T per active target."""
        for site, col in self.groups.get(group, ()):
            t = self._t_of(eng, site)
            ops.lora_down(x, site.A, t, M, site.K)
            ops.lora_up(y, t, site.B, M, site.N, alpha=self.s, y_off=col, w_nr=True)

    def backward(self, eng, group, dy, x, dx, M):
        """dy is final and the site's _dgrad has written (or accumulated) the base term of dx: dT = s dY B, dB = s dY^T t, dA = dT^T x, dx += dT A."""
        for site, col in self.groups.get(group, ()):
            dT, ws = self._scratch(eng, M, max(site.K, site.N))
            ops.lora_down(dy, site.B, dT, M, site.N, alpha=self.s, x_off=col, w_kr=True)
            ops.lora_wgrad(site.t, dy, site.gB, M, site.N, alpha=self.s, x_off=col, g_cr=True, ws=ws)
            ops.lora_wgrad(dT, x, site.gA, M, site.K, ws=ws)
            ops.lora_up(dx, dT, site.A, M, site.K)

    def head_ranges(self, eng):
        return [eng.slots[n] for n in ('head.w', 'head.b')] if self.train_heads else []

    def step(self, eng, lr, betas, eps, weight_decay, max_norm, gscale):
        """Clip norm over the adapter gradients (+ the head ranges), then pb_adamw_step on exactly those ranges; the bf16 shadow of the head ranges
        (and the transposed copy of head.w that the backward reads) is refreshed by the same pass. The backbone is never written."""
        heads = self.head_ranges(eng)
        if self.m is None:
            self.m, self.v = torch.zeros_like(self.P), torch.zeros_like(self.P)
        if heads and self.head_m is None:
            self.head_m = {i: torch.zeros(h.numel, dtype=torch.float32, device=eng.device) for i, h in enumerate(heads)}
            self.head_v = {i: torch.zeros(h.numel, dtype=torch.float32, device=eng.device) for i, h in enumerate(heads)}
        sq, clip, part = eng.scal[40:41], eng.scal[41:42], eng.scal[42:43]
        ops.grad_sqnorm(self.G, eng.partials, sq)
        for h in heads:
            ops.grad_sqnorm(eng.G32[h.off:h.off + h.numel], eng.partials, part)
            ops.accum_f32(sq, part, add=True)
        ops.clip_coef(sq, max_norm, gscale, clip)
        ops.adamw_step(self.P, self.G, self.m, self.v, None, clip, lr, betas[0], betas[1], eps, weight_decay, eng.step_count)
        for i, h in enumerate(heads):
            lo, hi = h.off, h.off + h.numel
            ops.adamw_step(eng.P32[lo:hi], eng.G32[lo:hi], self.head_m[i], self.head_v[i], eng.Pbf[lo:hi] if eng.Pbf is not None else None, clip, lr,
                           betas[0], betas[1], eps, weight_decay, eng.step_count)
        if heads and eng.Pbf is not None and 'head.w' in eng.wT:
            if self._head_table is None:
                h = eng.slots['head.w']
                R, C = h.shape
                self._head_table = (torch.tensor([[h.off, R, C, 0]], dtype=torch.int32, device=eng.device), -(-R // 64) * -(-C // 64))
            ops.transpose_batch_bf16(eng.Pbf, eng.PbfT, *self._head_table)

    def optimizer_numel(self):
        """Elements of optimizer state held while the adapters are attached."""
        n = 0 if self.m is None else self.m.numel() + self.v.numel()
        if self.head_m is not None:
            n += sum(t.numel() for t in self.head_m.values()) + sum(t.numel() for t in self.head_v.values())
        return n

    def merge(self, eng, sign=1.0):
        for s in self.sites:
            ops.lora_merge(eng.wf[s.slot][s.row:s.row + s.N], s.B, s.A, sign * self.s)


# ---- files ----------------------------------------------------------------------------------------------------------------------------------
def _engine_of(model):
    eng = model._get_engine() if hasattr(model, '_get_engine') else None
    if eng is None:
        raise PBError('lora: the model has no engine (a PianoBartLM is needed)')
    return eng


def _state_of(model):
    eng = _engine_of(model)
    if getattr(eng, 'lora', None) is None:
        raise PBError('lora: no adapters are attached to this model (Engine.attach_lora)')
    return eng, eng.lora


def _site_names(model, st):
    """{site: the module's parameter name without '.weight'}, e.g. pianobart.bart.decoder.layers.0.encoder_attn.v_proj."""
    name_of = {id(p): k for k, p in model.named_parameters()}
    out = {}
    for s in st.sites:
        k = name_of.get(id(s.module.weight))
        if k is None or not k.endswith('.weight'):
            raise PBError('lora: site %s is not a parameter of this model' % s.key)
        out[s.key] = k[:-len('.weight')]
    return out


def adapter_keys(model, cfg, train_heads=True):
    """{key: shape} of the tensors an adapter file of `model` under `cfg` holds: '<module name>.lora_A' (r, K) and '.lora_B' (N, r) per site,
    plus the mask_lm.* tensors when the heads train. Needs no device."""
    eng = _engine_of(model)
    cfg.check(eng.d)
    name_of = {id(p): k for k, p in model.named_parameters()}
    out = {}
    for _, _, s in _site_list(eng, cfg.targets):
        base = name_of[id(s.module.weight)][:-len('.weight')]
        out[base + '.lora_A'], out[base + '.lora_B'] = (int(cfg.rank), s.K), (s.N, int(cfg.rank))
    if train_heads:
        out.update({k: tuple(p.shape) for k, p in _head_items(model)})
    return out


def _model_shape(eng):
    return dict(d_model=int(eng.d), encoder_layers=int(eng.NE), decoder_layers=int(eng.ND), sizes=[int(n) for n in eng.lay.sizes])


def _head_items(model):
    return [(k, p) for k, p in model.named_parameters() if k.startswith('mask_lm.')]


def save(path, model):
    """Write the adapter file: the config, A / B per site under '<module name>.lora_A' / '.lora_B', the mask_lm.* tensors when the heads were
    trained, and the moments and step count of both. Never a backbone tensor."""
    eng, st = _state_of(model)
    names = _site_names(model, st)
    cpu = lambda t: t.detach().to('cpu', copy=True)
    sd, m, v = {}, {}, {}
    for s in st.sites:
        for tag, lo, shape in (('.lora_A', s.off_a, (st.r, s.K)), ('.lora_B', s.off_b, (s.N, st.r))):
            k, n = names[s.key] + tag, shape[0] * shape[1]
            sd[k] = cpu(st.P[lo:lo + n].view(shape))
            if st.m is not None:
                m[k], v[k] = cpu(st.m[lo:lo + n].view(shape)), cpu(st.v[lo:lo + n].view(shape))
    if st.train_heads:
        by_id = {id(p): (slot, row) for p, (slot, row) in zip(eng.params, eng.param_slots)}
        heads = st.head_ranges(eng)
        for k, p in _head_items(model):
            sd[k] = cpu(p)
            if st.head_m is not None:
                slot, row = by_id[id(p)]
                i = 0 if slot == 'head.w' else 1
                o = eng._elem_off(slot, row) - heads[i].off
                m[k], v[k] = cpu(st.head_m[i][o:o + p.numel()].view(p.shape)), cpu(st.head_v[i][o:o + p.numel()].view(p.shape))
    torch.save({'format': FORMAT, 'config': st.cfg.to_dict(), 'model': _model_shape(eng), 'train_heads': st.train_heads, 'state_dict': sd,
                'optimizer': {'step': int(eng.step_count), 'exp_avg': m or None, 'exp_avg_sq': v or None}}, path)


def read(path):
    f = torch.load(path, map_location='cpu', weights_only=False)
    if not isinstance(f, dict) or f.get('format') != FORMAT or 'state_dict' not in f:
        raise PBError('%s is not an adapter file written by pianobart_amd.lora.save' % path)
    return f


def check_file(f, shape):
    """PBError unless the adapter file `f` was written for a model of `shape` (_model_shape)."""
    fm = f.get('model', {})
    for k in ('d_model', 'encoder_layers', 'decoder_layers'):
        if fm.get(k) != shape[k]:
            raise PBError('the adapter was trained on a model with %s = %s, this model has %s' % (k, fm.get(k), shape[k]))
    if list(fm.get('sizes', [])) != list(shape['sizes']):
        raise PBError('the adapter was trained on the vocabulary layout %s, this model has %s' % (fm.get('sizes'), shape['sizes']))


def load(path, model, with_optimizer=True):
    """Attach the adapters of an adapter file to `model` (loaded from the base checkpoint the adapters were trained on) and restore A / B,
    the heads and the moments. Refuses a file whose d_model, layer counts or vocabulary layout differ from the model's."""
    f = read(path)
    eng = _engine_of(model)
    check_file(f, _model_shape(eng))
    cfg = LoraConfig(**f['config'])
    eng.attach_lora(cfg, seed=0, train_heads=bool(f.get('train_heads', False)))
    st = eng.lora
    names = _site_names(model, st)
    sd, opt = f['state_dict'], f.get('optimizer') or {}
    m, v = opt.get('exp_avg'), opt.get('exp_avg_sq')
    want = {names[s.key] + tag for s in st.sites for tag in ('.lora_A', '.lora_B')}
    got = {k for k in sd if k.endswith('.lora_A') or k.endswith('.lora_B')}
    if want != got:
        eng.detach_lora()
        raise PBError('the adapter file names %d matrices, the model\'s targets %d (first difference: %s)' % (len(got), len(want), sorted(want ^ got)[0]))
    if with_optimizer and m:
        st.m, st.v = torch.zeros_like(st.P), torch.zeros_like(st.P)
    with torch.no_grad():
        for s in st.sites:
            for tag, dst, lo in (('.lora_A', s.A, s.off_a), ('.lora_B', s.B, s.off_b)):
                k = names[s.key] + tag
                if tuple(sd[k].shape) != tuple(dst.shape):
                    eng.detach_lora()
                    raise PBError('adapter %s has shape %s, the model needs %s' % (k, tuple(sd[k].shape), tuple(dst.shape)))
                dst.copy_(sd[k])
                if with_optimizer and m:
                    st.m[lo:lo + dst.numel()].view(dst.shape).copy_(m[k])
                    st.v[lo:lo + dst.numel()].view(dst.shape).copy_(v[k])
        if st.train_heads:
            by_id = {id(p): (slot, row) for p, (slot, row) in zip(eng.params, eng.param_slots)}
            heads = st.head_ranges(eng)
            items = _head_items(model)
            if with_optimizer and m and all(k in m for k, _ in items):
                st.head_m = {i: torch.zeros(h.numel, dtype=torch.float32, device=eng.device) for i, h in enumerate(heads)}
                st.head_v = {i: torch.zeros(h.numel, dtype=torch.float32, device=eng.device) for i, h in enumerate(heads)}
            for k, p in items:
                if k not in sd:
                    eng.detach_lora()
                    raise PBError('the adapter file was written with trained heads but holds no %s' % k)
                p.data.copy_(sd[k])
                if st.head_m is not None:
                    slot, row = by_id[id(p)]
                    i = 0 if slot == 'head.w' else 1
                    o = eng._elem_off(slot, row) - heads[i].off
                    st.head_m[i][o:o + p.numel()].view(p.shape).copy_(m[k])
                    st.head_v[i][o:o + p.numel()].view(p.shape).copy_(v[k])
            eng.refresh_shadow(force=True)
    if with_optimizer:
        eng.step_count = int(opt.get('step', 0))
    return st


def merged_state_dict(model):
    """A plain whole-model state dict (CPU tensors) with every adapter folded into its weight, W + s B A by the kernel Engine.merge_lora runs.
    The live model keeps its adapters."""
    eng, st = _state_of(model)
    names = _site_names(model, st)
    sd = {k: v.detach().to('cpu', copy=True) for k, v in model.state_dict().items()}
    for s in st.sites:
        w = s.module.weight.detach().clone().contiguous()
        ops.lora_merge(w, s.B, s.A, st.s)
        sd[names[s.key] + '.weight'] = w.cpu()
    return sd


def merge_into_state_dict(sd, f, device):
    """Fold the adapters of adapter file `f` into the whole-model state dict `sd` (CPU tensors, keys as PianoBartLM names them) on `device`; the
    file's mask_lm.* tensors replace the checkpoint's. Returns a new dict."""
    out = dict(sd)
    cfg = LoraConfig(**f['config']).check()
    for k, A in f['state_dict'].items():
        if k.endswith('.lora_A'):
            base = k[:-len('.lora_A')]
            wk = base + '.weight'
            if wk not in sd:
                raise PBError('the checkpoint has no %s for adapter %s (is it the base the adapter was trained on?)' % (wk, k))
            B = f['state_dict'][base + '.lora_B']
            w = sd[wk].to(device=device, dtype=torch.float32).clone().contiguous()
            if tuple(w.shape) != (B.shape[0], A.shape[1]):
                raise PBError('%s is %s in the checkpoint, the adapter was trained on %s' % (wk, tuple(w.shape), (B.shape[0], A.shape[1])))
            ops.lora_merge(w, B.to(device).contiguous(), A.to(device).contiguous(), cfg.scale)
            out[wk] = w.cpu()
        elif not k.endswith('.lora_B'):
            out[k] = f['state_dict'][k].clone()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description='fold a LoRA adapter file into a whole checkpoint (the layout finetune_generation writes)')
    ap.add_argument('--ckpt', required=True, help='the base checkpoint the adapters were trained on')
    ap.add_argument('--lora', required=True, help='adapter file (model.lora.pt)')
    ap.add_argument('--output', required=True, help='merged checkpoint to write')
    ap.add_argument('--cuda_device', type=int, default=0)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise PBError('pianobart_amd has no CPU execution path: merging runs pb_lora_merge on the device')
    from .model import checkpoint_state_dict
    f = read(args.lora)
    ck = torch.load(args.ckpt, map_location='cpu', weights_only=False)
    sd = checkpoint_state_dict(ck['state_dict'])
    if sd and not any(k.startswith('pianobart.') for k in sd):           # a pre-train checkpoint holds the backbone alone
        sd = {'pianobart.' + k: v for k, v in sd.items()}
    merged = merge_into_state_dict(sd, f, torch.device('cuda', args.cuda_device))
    state = {k: v for k, v in ck.items() if k not in ('state_dict', 'optimizer')}
    state['state_dict'] = merged
    torch.save(state, args.output)
    print('wrote %s: %d tensors, %d adapters of rank %d merged' % (args.output, len(merged), sum(k.endswith('.lora_A') for k in f['state_dict']), f['config']['rank']))


if __name__ == '__main__':
    main()
