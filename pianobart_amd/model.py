"""Drop-in PianoBART classes for MI355X.

Same public surface as the reference (PianoBart.py:9-91, model.py:14-126): `Embeddings`, `PianoBart`,
`MLM`, `PianoBartLM`, `sampling`, `nucleus`, and the same `state_dict` layout. The
modules below only *hold* the parameters under the reference's names; all arithmetic runs in the
hand-written HIP kernels of libpianobart_hip.so through `pianobart_amd.engine.Engine`. There is no
CPU execution path: calling forward with CPU tensors raises.
"""
import math
import random
import threading
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import LIB, PBError

CLASSES = ['Bar', 'Position', 'Instrument', 'Pitch', 'Duration', 'Velocity', 'TimeSig', 'Tempo']


def checkpoint_state_dict(sd, module=None):
    """The `state_dict` of a reference checkpoint, ready for `load_state_dict`.

    Under `nn.DataParallel` the reference saves `self.model.state_dict()` of the WRAPPER (finetune_generation.py:276-285,
    finetune.py save_checkpoint), so every key carries a leading `module.`; its own `demo.py:128-129` then loads that file with
    `strict=False` and silently keeps the random initialisation. Here the prefix is stripped (with a message), and -- when `module`
    is given -- a file none of whose keys name a parameter of `module` is reported instead of being "loaded"."""
    if sd and all(k.startswith('module.') for k in sd):
        print("   [pianobart_amd] checkpoint was saved from an nn.DataParallel wrapper: stripping the 'module.' prefix of its %d keys" % len(sd))
        sd = type(sd)((k[len('module.'):], v) for k, v in sd.items())
    if module is not None:
        own = set(module.state_dict().keys())
        hit = sum(k in own for k in sd)
        if hit == 0:
            print("   [pianobart_amd] WARNING: none of the checkpoint's %d keys names a parameter of %s (first key: %r): nothing will be "
                  "loaded under strict=False" % (len(sd), type(module).__name__, next(iter(sd), None)))
    return sd


class BartConfig:
    """Stand-in for transformers.BartConfig with the attributes the reference reads (main.py:39-47 sets the
    first eight; the rest are BartConfig defaults). Any object with these attribute names is accepted."""

    def __init__(self, max_position_embeddings=1024, d_model=1024, encoder_layers=12, encoder_ffn_dim=4096,
                 encoder_attention_heads=16, decoder_layers=12, decoder_ffn_dim=4096, decoder_attention_heads=16,
                 vocab_size=50265, dropout=0.1, attention_dropout=0.0, activation_dropout=0.0,
                 activation_function="gelu", init_std=0.02, scale_embedding=False, pad_token_id=1, **kw):
        self.max_position_embeddings = max_position_embeddings
        self.d_model = d_model
        self.encoder_layers = encoder_layers
        self.encoder_ffn_dim = encoder_ffn_dim
        self.encoder_attention_heads = encoder_attention_heads
        self.decoder_layers = decoder_layers
        self.decoder_ffn_dim = decoder_ffn_dim
        self.decoder_attention_heads = decoder_attention_heads
        self.vocab_size = vocab_size
        self.dropout = dropout
        self.attention_dropout = attention_dropout
        self.activation_dropout = activation_dropout
        self.activation_function = activation_function
        self.init_std = init_std
        self.scale_embedding = scale_embedding
        self.pad_token_id = pad_token_id
        for k, v in kw.items():
            setattr(self, k, v)


# ---- parameter containers named exactly like transformers' BartModel (modeling_bart.py) -------------
class _Attention(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.k_proj = nn.Linear(d, d)
        self.v_proj = nn.Linear(d, d)
        self.q_proj = nn.Linear(d, d)
        self.out_proj = nn.Linear(d, d)


class _EncLayer(nn.Module):
    def __init__(self, d, f):
        super().__init__()
        self.self_attn = _Attention(d)
        self.self_attn_layer_norm = nn.LayerNorm(d)
        self.fc1 = nn.Linear(d, f)
        self.fc2 = nn.Linear(f, d)
        self.final_layer_norm = nn.LayerNorm(d)


class _DecLayer(nn.Module):
    def __init__(self, d, f):
        super().__init__()
        self.self_attn = _Attention(d)
        self.self_attn_layer_norm = nn.LayerNorm(d)
        self.encoder_attn = _Attention(d)
        self.encoder_attn_layer_norm = nn.LayerNorm(d)
        self.fc1 = nn.Linear(d, f)
        self.fc2 = nn.Linear(f, d)
        self.final_layer_norm = nn.LayerNorm(d)


class _Stack(nn.Module):
    def __init__(self, cfg, shared, decoder):
        super().__init__()
        d = cfg.d_model
        self.embed_tokens = shared      # dead 50265 x d table kept for checkpoint compatibility (never read)
        self.embed_positions = nn.Embedding(cfg.max_position_embeddings + 2, d)
        if decoder:
            self.layers = nn.ModuleList([_DecLayer(d, cfg.decoder_ffn_dim) for _ in range(cfg.decoder_layers)])
        else:
            self.layers = nn.ModuleList([_EncLayer(d, cfg.encoder_ffn_dim) for _ in range(cfg.encoder_layers)])
        self.layernorm_embedding = nn.LayerNorm(d)


class _BartParams(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.shared = nn.Embedding(cfg.vocab_size, cfg.d_model, padding_idx=cfg.pad_token_id)
        self.encoder = _Stack(cfg, self.shared, decoder=False)
        self.decoder = _Stack(cfg, self.shared, decoder=True)
        std = cfg.init_std
        for m in self.modules():            # BartPreTrainedModel._init_weights distributions
            if isinstance(m, nn.Linear):
                m.weight.data.normal_(0.0, std)
                m.bias.data.zero_()
            elif isinstance(m, nn.Embedding):
                m.weight.data.normal_(0.0, std)
                if m.padding_idx is not None:
                    m.weight.data[m.padding_idx].zero_()


class Embeddings(nn.Module):
    """PianoBart.py:9-16 (parameter holder; lut(x)*sqrt(d_model) is folded into the projected table)."""

    def __init__(self, n_token, d_model):
        super().__init__()
        self.lut = nn.Embedding(n_token, d_model)
        self.d_model = d_model

    def forward(self, x):
        """lut(x) * sqrt(d_model) (PianoBart.py:15-16) for direct callers: a HIP row gather + scale, differentiable in `lut`. Inside
        PianoBart.forward the eight embeddings never run on their own: they are folded into the projected Octuple table."""
        from . import heads
        e = heads.gather_rows(self.lut.weight, x)
        return heads.mul(e, torch.full_like(e, math.sqrt(self.d_model)))


def _check_cfg(cfg):
    d = cfg.d_model
    if d % 4 != 0 or d > 2048:
        raise PBError('d_model=%d unsupported by the HIP row kernels (need a multiple of 4, <= 2048)' % d)
    if cfg.encoder_attention_heads != cfg.decoder_attention_heads or d % cfg.encoder_attention_heads != 0:
        raise PBError('encoder/decoder head counts must match and divide d_model')
    if (d // cfg.encoder_attention_heads) % 8 != 0:
        raise PBError('head_dim must be a multiple of 8')
    if getattr(cfg, 'activation_function', 'gelu') != 'gelu':
        raise PBError('only the exact-erf "gelu" activation of the reference is implemented')
    if getattr(cfg, 'attention_dropout', 0.0) != 0.0 or getattr(cfg, 'activation_dropout', 0.0) != 0.0:
        raise PBError('attention_dropout / activation_dropout must be 0 (reference defaults)')
    if getattr(cfg, 'scale_embedding', False):
        raise PBError('scale_embedding=True is not used by the reference and not implemented')


class PianoBart(nn.Module):
    """PianoBart.py:19-91. `precision`: "bf16" (throughput, bf16 MFMA), "fp32" (exact-f32 parity path) or "bf16x3" (f32 storage and row
    kernels, every GEMM as split-bf16 triples on the bf16 matrix cores: parity-grade at a multiple of the f32-MFMA rate)."""

    def __init__(self, bartConfig, e2w, w2e, precision='bf16'):
        super().__init__()
        _check_cfg(bartConfig)
        # the vocabulary layout is the dictionary's (ops.Layout): an illegal dictionary is refused here, by head and rule, before any device work
        object.__setattr__(self, 'layout', ops.Layout.from_dict(e2w))
        self.bart = _BartParams(bartConfig)
        self.hidden_size = bartConfig.d_model
        self.bartConfig = bartConfig
        self.n_tokens = []
        self.classes = list(CLASSES)
        for key in self.classes:
            self.n_tokens.append(len(e2w[key]))
        self.emb_sizes = [256] * 8
        self.e2w = e2w
        self.w2e = w2e
        self.bar_pad_word = self.e2w['Bar']['Bar <PAD>']
        mk = lambda tag: np.array([self.e2w[e]['%s <%s>' % (e, tag)] for e in self.classes], dtype=np.int64)
        self.mask_word_np = mk('MASK')
        self.pad_word_np = mk('PAD')
        self.sos_word_np = mk('SOS')
        self.eos_word_np = mk('EOS')
        self.word_emb = nn.ModuleList([Embeddings(self.n_tokens[i], self.emb_sizes[i]) for i in range(8)])
        self.encoder_linear = nn.Linear(int(np.sum(self.emb_sizes)), bartConfig.d_model)
        self.decoder_linear = self.encoder_linear
        self.decoder_emb = None
        self.precision = precision
        object.__setattr__(self, '_engine', None)
        object.__setattr__(self, '_engine_owner', None)

    # -- engine plumbing ---------------------------------------------------------------------
    def _get_engine(self):
        if self._engine_owner is not None:
            return self._engine_owner._get_engine()
        if self._engine is None:
            from .engine import Engine
            object.__setattr__(self, '_engine', Engine(self, None, self.precision))
        return self._engine

    def forward(self, input_ids_encoder, input_ids_decoder=None, encoder_attention_mask=None,
                decoder_attention_mask=None, output_hidden_states=True, generate=False):
        eng = self._get_engine()
        if self.decoder_emb is not None and input_ids_decoder is not None:
            # PianoBart.py:65-66,71: decoder_linear(decoder_emb(labels)) with Embeddings = lut(x) * sqrt(d_model) -- computed as a
            # row gather from the projected label table sqrt(d_model) * lut @ W^T (n_labels x d), differentiable in lut, W and b
            from . import heads
            table = heads.linear(self.decoder_emb.lut.weight, self.decoder_linear.weight, None, alpha=math.sqrt(self.decoder_emb.d_model))
            e = heads.gather_rows(table, input_ids_decoder, self.decoder_linear.bias)
            dec_h, enc_h = eng.module_forward_hidden(input_ids_encoder, None, encoder_attention_mask, decoder_attention_mask, self.training,
                                                     dec_embeds=e)
            return SimpleNamespace(last_hidden_state=dec_h, encoder_last_hidden_state=enc_h)
        dec_h, enc_h = eng.module_forward_hidden(input_ids_encoder, input_ids_decoder, encoder_attention_mask,
                                                 decoder_attention_mask, self.training)
        if input_ids_decoder is None:
            return SimpleNamespace(last_hidden_state=enc_h)
        return SimpleNamespace(last_hidden_state=dec_h, encoder_last_hidden_state=enc_h)

    def embed(self, input_ids_encoder, encoder_attention_mask=None, return_counts=False):
        """One vector per piece: the encoder's last hidden state mean-pooled over the rows whose mask is not 0 (None: every row), a (B, d)
        float32 device tensor (embedding.py). One encoder-only forward without dropout and without an autograd graph, in the
        model's own precision; the sum over the rows runs in float64 in a fixed order (pb_pool_rows). A row with no visible position gives a
        zero vector; return_counts=True returns (emb, count) with count (B) int32 = the pooled rows of each piece."""
        ids = torch.as_tensor(input_ids_encoder)
        if ids.dim() != 3 or int(ids.shape[2]) != 8 or ids.dtype.is_floating_point or ids.dtype == torch.bool:
            raise PBError('embed: input_ids_encoder must be (B, S, 8) integers (got %s %s)' % (tuple(ids.shape), ids.dtype))
        if ids.device.type != 'cuda':
            raise PBError('pianobart_amd needs HIP device tensors (got %s); there is no CPU path' % ids.device)
        emb, count = self._get_engine().embed(ops.ids_to_i16(ids), encoder_attention_mask)
        return (emb, count) if return_counts else emb

    def get_rand_tok(self):
        rand = [0] * 8
        for i in range(8):
            rand[i] = random.choice(range(self.n_tokens[i]))
        return np.array(rand)

    def change_decoder_embedding(self, new_embedding, new_linear=None):
        self.decoder_emb = new_embedding
        if new_linear is not None:
            self.decoder_linear = new_linear


class MLM(nn.Module):
    """model.py:109-126 (parameter holder; the 8 heads run as one fused d x vocab GEMM, vocab = 1280 for the default dictionary)."""

    def __init__(self, e2w, n_tokens, hidden_size):
        super().__init__()
        self.proj = nn.ModuleList([nn.Linear(hidden_size, n_tokens[i]) for i, _ in enumerate(e2w)])
        self.e2w = e2w

    def forward(self, y):
        """model.py:119-126 for direct callers: y = pianobart(...) output (anything with .last_hidden_state) or a (B,S,d) tensor ->
        list of 8 (B,S,n_i) f32 logits through the exact-f32 HIP GEMM. PianoBartLM.forward runs the 8 heads as ONE fused GEMM instead."""
        from . import heads
        h = y.last_hidden_state if hasattr(y, 'last_hidden_state') else y
        return [heads.linear(h, self.proj[i].weight, self.proj[i].bias) for i, _ in enumerate(self.e2w)]


# -- nucleus sampling: host-side numpy exactly like the reference, so the RNG stream matches ----------
def nucleus(probs, p):
    """model.py:84-98 (mutates probs in place; draws from the global np.random)."""
    probs /= (sum(probs) + 1e-5)
    sorted_probs = np.sort(probs)[::-1]
    sorted_index = np.argsort(probs)[::-1]
    cusum_sorted_probs = np.cumsum(sorted_probs)
    after_threshold = cusum_sorted_probs > p
    if sum(after_threshold) > 0:
        last_index = np.where(after_threshold)[0][0] + 1
        candi_index = sorted_index[:last_index]
    else:
        candi_index = sorted_index[0:1]
    candi_probs = [probs[i] for i in candi_index]
    candi_probs /= sum(candi_probs)
    word = np.random.choice(candi_index, size=1, p=candi_probs)[0]
    return word


_SAMPLE_TLS = threading.local()


def _sample_tables(layout=None):
    """Constants and scratch of PianoBartLM.sample_row for one vocabulary layout: per-element temperatures, the (8, width) probability rows
    (width = the largest head rounded up to 16: 272 for the default dictionary), the native call's arrays. One set per thread and layout:
    Engine.generate_batch verifies the rows of a batch on a small thread pool."""
    layout = layout or ops.DEFAULT_LAYOUT
    tabs = getattr(_SAMPLE_TLS, 'tabs', None)
    if tabs is None:
        tabs = _SAMPLE_TLS.tabs = {}
    tab = tabs.get(layout)
    if tab is None:
        tab = tabs[layout] = {}
        n = list(layout.sizes)
        width = (max(n) + 15) // 16 * 16
        n_a, p_a = np.asarray(n, dtype=np.int32), np.asarray(PianoBartLM.SAMPLE_P, dtype=np.float32)
        tab.update(n_a=n_a, p_a=p_a, n_p=n_a.ctypes.data, p_p=p_a.ctypes.data, out=np.zeros(8, dtype=np.int32), tie=np.zeros(1, dtype=np.int32))
        tab.update(n=n, probs=torch.zeros(8, width, dtype=torch.float32),
                   tvec=torch.cat([torch.full((n[j],), float(PianoBartLM.SAMPLE_T[j]), dtype=torch.float32) for j in range(8)]))
    return tab


def _nucleus_with_draw(probs, p, u):
    """_nucleus_fast with the uniform draw handed in (PianoBartLM.sample_row draws the 8 of a position at once)."""
    probs = probs / (np.cumsum(probs)[-1] + 1e-5)
    order = np.argsort(probs)[::-1]
    after = np.cumsum(probs[order]) > p
    cand = order[:int(np.argmax(after)) + 1] if after.any() else order[0:1]
    q = probs[cand]
    q = q / np.cumsum(q)[-1]
    cdf = q.astype(np.float64).cumsum()
    cdf /= cdf[-1]
    return int(cand[int(cdf.searchsorted(u, side='right'))])


def _nucleus_fast(probs, p):
    """The same draw as nucleus() for the same probs / global np.random state, without its Python-level loops: builtin sum() over a
    float32 array is a left-to-right float32 accumulation = np.cumsum(..)[-1]; np.random.choice(c, size=1, p=q) is, in RandomState,
    cdf = q.astype(f64).cumsum(); cdf /= cdf[-1]; c[cdf.searchsorted(random_sample(1), 'right')]. Checked draw for draw (values and
    RNG stream) against nucleus() in tests/test_model_cpu.py; 0.30 -> 0.1 ms of host time per generated position."""
    probs /= (np.cumsum(probs)[-1] + 1e-5)
    order = np.argsort(probs)[::-1]
    after = np.cumsum(probs[order]) > p
    cand = order[:int(np.argmax(after)) + 1] if after.any() else order[0:1]
    q = probs[cand]
    q = q / np.cumsum(q)[-1]
    cdf = q.astype(np.float64).cumsum()
    cdf /= cdf[-1]
    return cand[int(cdf.searchsorted(np.random.random_sample(1), side='right')[0])]


def sampling(logit, p=None, t=1.0):
    """model.py:101-107."""
    logit = logit.squeeze()
    probs = torch.softmax(logit / t, dim=-1)
    probs = probs.cpu().detach().numpy()
    return nucleus(probs, p=p)


class PianoBartLM(nn.Module):
    """model.py:14-78. Train branch returns a mutable list of 8 (B,S,n_i) f32 tensors with autograd;
    generate=True runs the KV-cached HIP decode (same tokens as the reference's full re-run)."""

    def __init__(self, pianobart: PianoBart):
        super().__init__()
        self.pianobart = pianobart
        self.mask_lm = MLM(self.pianobart.e2w, self.pianobart.n_tokens, self.pianobart.hidden_size)
        object.__setattr__(self, '_engine', None)
        # plain attribute (bypass nn.Module registration: the LM must not become a child of its child)
        object.__setattr__(pianobart, '_engine_owner', self)
        object.__setattr__(pianobart, '_engine', None)

    def _get_engine(self):
        if self._engine is None:
            from .engine import Engine
            object.__setattr__(self, '_engine', Engine(self.pianobart, self.mask_lm, self.pianobart.precision))
        return self._engine

    def forward(self, input_ids_encoder, input_ids_decoder=None, encoder_attention_mask=None,
                decoder_attention_mask=None, generate=False, device_num=-1, *, decoder_prefix=None, decoder_forced=None, decoder_stop=None,
                decoder_order=None, decoder_allow=None, decoder_bar_allow=None, decoder_anchors=None):
        """decoder_prefix (1, k, 8) (generate=True only): primed generation -- the first k decoder events are given and the loop samples from
        position k on (Engine.generate's `prefix`).
        decoder_forced (1, S, 8) integers in model column order (generate=True only): forced tokens -- -1 leaves a head free, v >= 0 says
        "head h of position i is v" (generation.keep_mask builds the table from a piece). The result is the reference loop
        (model.py:42-65) with the given heads of `current_output` overwritten right after `self.sample(x, i)`: the stop rule sees the token
        after forcing (a given special id ends the piece there, a given ordinary id keeps it going where the sample would have been
        special); a position with a free head draws its 8 uniforms as ever (the draws of its given heads are consumed and unused), a
        position whose 8 heads are given draws nothing; a given id may be any id of its head's table (IndexError otherwise); positions
        inside decoder_prefix must be -1 (PBError). None, or -1 everywhere, is the call without the argument.
        decoder_stop (a bar id 0 .. the bar head's PAD id, 256 in the default dictionary, or a sequence of one; generate=True only): stop at a bar -- the reference loop with its stop test
        `(current_output >= pad).any()` replaced by `(current_output >= pad).any() or current_output[0] >= decoder_stop`. The test sees the
        token after forcing; the token that trips it is not written and its draws are consumed; positions inside decoder_prefix are not
        tested (generation.stop_after_bars turns "n more bars" into the bar id). 256 (the bar head's PAD id), or None: no stop.
        decoder_order (-1 .. the bar head's PAD id - 1, 255 in the default dictionary, or a sequence of one; generate=True only): time-ordered sampling -- the reference loop with `current_output
        = self.sample(x, i)` replaced by a sample whose (bar, position) never goes back. With prev = the decoder's input row of position i
        (the SOS row, the prefix's last row, else the previous token after forcing): bars below max(decoder_order, prev's bar) have
        probability 0, and so have positions below prev's position while the bar (after forcing) stays prev's. Special ids stay
        reachable, heads 2 .. 7 and given heads are untouched, and the draws are those of the unordered call. 0 = ordered without an
        extra bar floor; -1, or None: not ordered. DESIGN.md section 1, "Time-ordered sampling".
        decoder_allow ((V,) bools in model column order, V = the layout's total, 1280 in the default dictionary, or a sequence of one;
        generate=True only): allowed classes -- the reference loop with `sampling(logit, p, t)` seeing -inf in place of every logit whose
        bit is False: such a class has probability exactly 0, is never a nucleus candidate and never the arg-max of a p = 1 head. The
        mask is constant over the positions; the six special ids of every head are always reachable (generation.check_allow sets them);
        given heads are written as given; the draws, the stop test and decoder_prefix are untouched; with decoder_order the row loses the
        classes either rule removes. generation.allow_mask builds a mask from the dictionary's names (key, pitch range, instruments, ..).
        None, or True everywhere: the call without the argument. DESIGN.md section 1, "Allowed classes".
        decoder_bar_allow (a bar schedule, or a sequence of one; generate=True only): a dict {bar id: (V,) bool mask} or a sequence of at
        most pad[0] masks / None indexed by bar id -- allowed classes that change with the bar. Head 0 (the bar) is sampled as without
        it; with b0 = head 0's id after forcing, heads 1 .. 7 of the token are sampled from `decoder_allow AND schedule[b0]` where b0 is
        an ordinary bar with an entry, else from decoder_allow alone. The special ids stay reachable; given heads, the draws, the stop
        test and the prefix are untouched; on an ordered row head 1's second pass starts from the bar's quotients.
        generation.chord_schedule builds one from chord names ('C:maj', 'G:maj', ..). None, no entry, or entries True everywhere: the
        call without the argument. DESIGN.md section 1, "Bar schedules".
        decoder_anchors (one (n, 8) array of complete Octuple rows, or a sequence of one; generate=True only): anchored notes -- the rows
        are kept wherever they fall in time and the model writes the notes around them ("harmonise this melody", "keep the bass line").
        Ordinary ids, non-decreasing in (bar, position). Every position is sampled as without them (the candidate); while anchors remain,
        a candidate that would end the row or whose (bar, position) has reached the next anchor's gives way to that anchor, all 8 heads as
        given (on a tie the anchor goes first; the candidate's draws stay consumed), so every anchor is written in order unless the
        window ends first, and the row cannot end while one remains. The row is time-ordered with floor max(decoder_order, 0). Not with
        decoder_forced. generation.anchor_rows picks a piece's skyline or bass line. None, or an empty list: the call without the
        argument. DESIGN.md section 1, "Anchored notes"."""
        eng = self._get_engine()
        if not generate:
            if decoder_prefix is not None:
                raise PBError('decoder_prefix primes generation: it needs generate=True')
            if decoder_forced is not None:
                raise PBError('decoder_forced gives tokens of a generated piece: it needs generate=True')
            if decoder_stop is not None:
                raise PBError('decoder_stop ends a generated piece at a bar: it needs generate=True')
            if decoder_order is not None:
                raise PBError('decoder_order constrains what a generated piece samples: it needs generate=True')
            if decoder_allow is not None:
                raise PBError('decoder_allow constrains what a generated piece samples: it needs generate=True')
            if decoder_bar_allow is not None:
                raise PBError('decoder_bar_allow constrains what a generated piece samples: it needs generate=True')
            if decoder_anchors is not None:
                raise PBError('decoder_anchors are notes a generated piece keeps: they need generate=True')
            logits = eng.module_forward_logits(input_ids_encoder, input_ids_decoder, encoder_attention_mask,
                                               decoder_attention_mask, self.training)
            off = self.pianobart.layout.seg_off
            return [logits[..., off[i]:off[i + 1]] for i in range(8)]
        if input_ids_encoder.shape[0] != 1:
            print("ERROR")
            exit(-1)
        out = eng.generate(input_ids_encoder, encoder_attention_mask, self.sample_row, sampler=dict(T=self.SAMPLE_T, P=self.SAMPLE_P),
                           prefix=decoder_prefix, forced=decoder_forced, stop=decoder_stop, order=decoder_order, allow=decoder_allow,
                           bar_allow=decoder_bar_allow, anchors=decoder_anchors)
        # model.py:33-36: the result lives on `cuda:device_num`, or on the CPU for device_num == -1
        return out.cpu() if device_num == -1 else out.to(torch.device('cuda', device_num))

    def generate_batch(self, input_ids_encoder, encoder_attention_mask=None, seeds=None, rngs=None, max_new=None, device_num=-1, *,
                       decoder_prefix=None, prefix_len=None, samples_per_prompt=None, decoder_forced=None, refill=False,
                       decoder_stop=None, decoder_order=None, decoder_allow=None, decoder_bar_allow=None, decoder_anchors=None):
        """Generation for B prompts at once (forward(generate=True) keeps the reference's batch-1 rule). Prompt b samples from its own
        numpy RandomState: rngs[b] (advanced in place) or RandomState(seeds[b]); one of the two is required. Row b of the (B, S, 8)
        result is what forward(generate=True) returns for prompt b alone after np.random.set_state(<that generator's state>); the global
        np.random stream is not touched. Placed like forward(generate=True): CPU for device_num == -1, else cuda:device_num.
        decoder_prefix (B, P, 8) + prefix_len (B lengths, None = P): prompt b is primed with its first prefix_len[b] rows, as
        forward(generate=True, decoder_prefix=...) primes one prompt; length 0 = unprimed.
        samples_per_prompt (an int n >= 1, or one int >= 1 per prompt): several continuations of each prompt. input_ids_encoder, the mask,
        decoder_prefix and prefix_len then describe P prompts, seeds / rngs hold R = sum(n_p) generators in prompt-major order (prompt 0's
        samples first) and the result is (R, S, 8) in that order, every row under the contract above with its own generator. The samples
        of a prompt share its encoder pass, cross-attention K/V and prefill (Engine.generate_batch's `samples`); None: one row per prompt.
        decoder_forced (B, S, 8), -1 = free: forced tokens, prompt b under forward(generate=True, decoder_forced=...)'s contract with its
        own table (rows that are -1 everywhere are unforced rows; positions below prefix_len[b] must be -1; max_new counts positions from
        prefix_len[b] on, given or sampled). With samples_per_prompt it describes the P prompts, like decoder_prefix. The given heads are
        applied inside the fused decoder's device sampler, so a forced batch keeps the batched decode's launches per step.
        refill (False, True or a slot count 2 .. 16): one decoder for the whole call whose rows are handed to the next waiting prompt as
        they stop (Engine.generate_batch's `refill`); the result is that of refill=False. Not with samples_per_prompt.
        decoder_stop (B bar ids 0 .. 256): prompt b under forward(generate=True, decoder_stop=...)'s contract with its own bar; 256 = no
        stop, so one batch may mix both. With samples_per_prompt it describes the P prompts. The fused decoder's device sampler makes the
        test too, so a stopped row leaves the batch (or frees its slot under refill) at once.
        decoder_order (B ints -1 .. 255): prompt b under forward(generate=True, decoder_order=...)'s contract with its own bar floor; -1 = not
        ordered, so one batch may mix both. With samples_per_prompt it describes the P prompts. The fused decoder's device sampler
        applies the same mask, so an ordered batch keeps the batched decode's launches per step and its rewind rate.
        decoder_allow ((B, V) bools, or a list of B entries, each a (V,) mask or None = free): prompt b under forward(generate=True,
        decoder_allow=...)'s contract with its own mask, so one batch may mix masked and free rows. With samples_per_prompt it describes
        the P prompts. The fused decoder's device sampler tests the same bits, so a masked batch keeps the batched decode's launches per
        step and its rewind rate.
        decoder_bar_allow (a list of B entries, each a bar schedule -- forward(generate=True, decoder_bar_allow=...)'s dict or sequence --
        or None): prompt b under that contract with its own schedule, so one batch may mix scheduled, masked and free rows. With
        samples_per_prompt it describes the P prompts. The device sampler picks the mask of heads 1 .. 7 by the bar it sampled, so a
        scheduled batch keeps the batched decode's launches per step and its rewind rate.
        decoder_anchors (a list of B entries, each an (n, 8) anchor list or None = a free prompt): prompt b under forward(generate=True,
        decoder_anchors=...)'s contract with its own anchors, so one batch may mix anchored and free rows. With samples_per_prompt it
        describes the P prompts. The device sampler applies the rule itself and keeps each row's counter, which a rewind restores."""
        B = int(input_ids_encoder.shape[0])
        if (rngs is None) == (seeds is None):
            raise PBError('generate_batch: give either seeds or rngs (one generator per prompt)')
        if rngs is None:
            rngs = [np.random.RandomState(int(s)) for s in seeds]
        rngs = list(rngs)
        from .generation import check_refill
        check_refill(refill, samples_per_prompt)
        if samples_per_prompt is not None:
            from .generation import check_samples
            check_samples(samples_per_prompt, B, len(rngs))
        elif len(rngs) != B:
            raise PBError('generate_batch: %d generators for %d prompts' % (len(rngs), B))
        eng = self._get_engine()
        out = eng.generate_batch(input_ids_encoder, encoder_attention_mask, self.sample_row, rngs, max_new=max_new,
                                 sampler=dict(T=self.SAMPLE_T, P=self.SAMPLE_P), prefix=decoder_prefix, prefix_len=prefix_len,
                                 samples=samples_per_prompt, forced=decoder_forced, refill=refill, stop=decoder_stop, order=decoder_order,
                                 allow=decoder_allow, bar_allow=decoder_bar_allow, anchors=decoder_anchors)
        return out.cpu() if device_num == -1 else out.to(torch.device('cuda', device_num))

    def embed(self, input_ids_encoder, encoder_attention_mask=None, return_counts=False):
        """PianoBart.embed of the backbone: one (d) float32 vector per piece."""
        return self.pianobart.embed(input_ids_encoder, encoder_attention_mask, return_counts)

    def score(self, input_ids_encoder, target_ids, encoder_attention_mask=None, start=None, length=None, device_num=-1):
        """Teacher-forced scores of B pieces (scoring.py; the forward-only quantity of Ablation.py:126-166): what the model thinks of
        target_ids (B, S, 8) as decoder output for the encoder input input_ids_encoder (B, S, 8). Position i of row b is scored iff
        start_b <= i < length_b. Defaults: length_b = the leading rows of target_ids[b] whose bar id is not the bar PAD (for a
        generate_batch result the row's emitted length), start_b = 0 (for a primed row pass its prefix length: forced positions are then
        not scored). Special ids (the EOS row of a dataset piece) are legal targets; an id outside its table raises IndexError.
        Returns a SimpleNamespace of tensors: logp, entropy (B, S, 8) f32 and rank (B, S, 8) int16 (0 / 0 / -1 where not scored),
        sum_logp, sum_entropy, hits (B, 8) f32 (hits = scored positions whose target is the head's argmax) and count (B,) f32 =
        scored positions. Placed like generate_batch: CPU for device_num == -1, else cuda:device_num. The argument rules
        (scoring.check_score_args) raise PBError before any device work."""
        from .scoring import check_score_args
        start, length = check_score_args(input_ids_encoder, target_ids, start, length, self.pianobart.bartConfig.max_position_embeddings,
                                         self.pianobart.bar_pad_word)
        if input_ids_encoder.device.type != 'cuda':
            raise PBError('pianobart_amd needs HIP device tensors (got %s); there is no CPU path' % input_ids_encoder.device)
        eng = self._get_engine()
        r = eng.score(ops.ids_to_i16(input_ids_encoder), ops.ids_to_i16(torch.as_tensor(target_ids).to(input_ids_encoder.device)), encoder_attention_mask,
                      start, length)
        dst = torch.device('cpu') if device_num == -1 else torch.device('cuda', device_num)
        return SimpleNamespace(**{k: v.to(dst) for k, v in vars(r).items()})

    # model.py:68-78 -- temperatures / nucleus thresholds per head
    SAMPLE_T =[1.2, 1.2, 5, 1, 2, 5, 5, 1.2]
    SAMPLE_P = [1, 1, 1, 0.9, 0.9, 1, 1, 0.9]

    def sample_row(self, row_logits, rng=None, order=None, allow=None, sched=None):
        """row_logits: (vocab,) f32 CPU tensor of one position (1280 for the default dictionary); returns the 8 sampled ids (model.py:68-78). sampling()'s own tensor ops
        on the host row -- the division by the temperature (one call with a per-element temperature vector: the same quotients) and a
        1-D softmax per head -- then nucleus() for all 8 heads in one native call (pb_nucleus_rows: numpy's arithmetic order and
        precision; ties among candidates go back to the numpy code), fed the 8 uniform draws np.random.choice would have made. Checked
        draw for draw and RNG state for RNG state against sampling() in tests/test_model_cpu.py. 0.31 -> 0.1 ms of host time per
        generated position, which sits in series with the GPU's ~0.3 ms. rng: a numpy RandomState to draw the 8 uniforms from instead of
        the global stream (generate_batch: one generator per prompt).
        order = (low, prev0, low1, given0) (generation.ordered_token), or None: the time-ordered sample. The quotients of head 0's
        classes below `low` are set to -inf in front of the softmax (probability exactly 0). If low1 > 0 and head 0's id after forcing
        (given0 if >= 0, else the id just sampled) equals prev0, head 1's classes below low1 are masked the same way and head 1 is sampled
        again with the same u[1]. One random_sample(8) either way; without `order` the arithmetic and the native call are unchanged.
        allow = a (vocab,) bool tensor or array, True = the class may be sampled (generation.allowed_token), or None: the quotients of
        the other columns are set to -inf in front of the 8 softmaxes (probability exactly 0), beside the ordered sample's own mask; head
        1's second pass starts from the masked quotients. The native call and the tie rule are unchanged; without `allow` so is the
        arithmetic.
        sched = (masks_by_bar, given0) (generation.scheduled_token), or None: the bar schedule. masks_by_bar[k] is the (vocab,) bool mask
        in force for heads 1 .. 7 of a token of bar k (already intersected with `allow`, special ids set), or None = `allow` alone. The
        position is sampled as without it; then, with b0 = head 0's id after forcing (given0 if >= 0, else the id just sampled), where b0
        is an ordinary bar with a mask the raw quotients of heads 1 .. 7 are masked with it, softmaxed again and pb_nucleus_rows runs
        again with the same u: out[0] is kept, heads 1 .. 7 are replaced. The ordered head-1 pass then starts from those quotients. One
        random_sample(8) either way; without `sched` the arithmetic and the native call are unchanged."""
        lay = getattr(getattr(self, 'pianobart', None), 'layout', None) or ops.DEFAULT_LAYOUT      # called on the class itself: the default dictionary
        tab = _sample_tables(lay)
        off = lay.seg_off
        y = row_logits / tab['tvec']
        probs = tab['probs']
        if allow is not None:
            y.masked_fill_(~torch.as_tensor(allow), -np.inf)
        if order is not None and order[0] > 0:
            y[off[0]:off[0] + order[0]] = -np.inf
        for j in range(8):                                           # 1-D calls: a 2-D softmax would open an OpenMP region per position
            torch.softmax(y[off[j]:off[j + 1]], dim=-1, out=probs[j, :tab['n'][j]])
        # the 8 draws np.random.choice would make, in head order (RandomState fills a request sequentially: the same stream as 8 calls)
        u = np.random.random_sample(8) if rng is None else rng.random_sample(8)
        out, tie = tab['out'], tab['tie']
        LIB.call('pb_nucleus_rows', probs.data_ptr(), probs.shape[1], tab['n_p'], tab['p_p'], u.ctypes.data, 8, out.ctypes.data, tie.ctypes.data)
        if tie[0]:                                                   # equal probabilities among a head's candidates: numpy's own order decides
            pn = probs.numpy()
            for j in range(8):
                if tie[0] >> j & 1:
                    out[j] = _nucleus_with_draw(pn[j, :tab['n'][j]], self.SAMPLE_P[j], u[j])
        if sched is not None:
            b0 = int(sched[1]) if sched[1] >= 0 else int(out[0])
            m = sched[0][b0] if b0 < len(sched[0]) else None         # a special bar id has no entry: the row ends
            if m is not None:
                # heads 1 .. 7 again under bar b0's mask (a subset of `allow`, so masking the quotients in place is masking the raw ones);
                # head 0's row of `probs` is untouched, so its id comes out as it did and is kept anyway
                y[off[1]:].masked_fill_(~torch.as_tensor(m)[off[1]:], -np.inf)
                for j in range(1, 8):
                    torch.softmax(y[off[j]:off[j + 1]], dim=-1, out=probs[j, :tab['n'][j]])
                again = out.copy()
                LIB.call('pb_nucleus_rows', probs.data_ptr(), probs.shape[1], tab['n_p'], tab['p_p'], u.ctypes.data, 8, again.ctypes.data, tie.ctypes.data)
                for j in range(1, 8):
                    out[j] = _nucleus_with_draw(probs.numpy()[j, :tab['n'][j]], self.SAMPLE_P[j], u[j]) if tie[0] >> j & 1 else again[j]
        if order is not None and order[2] > 0 and (order[3] if order[3] >= 0 else int(out[0])) == order[1]:
            # the token stays in its predecessor's bar: head 1 again, from the masked quotients, with the draw it had (the other rows of
            # `probs` are untouched, so their ids come out as they did)
            y[off[1]:off[1] + order[2]] = -np.inf
            torch.softmax(y[off[1]:off[2]], dim=-1, out=probs[1, :tab['n'][1]])
            head1 = out.copy()
            LIB.call('pb_nucleus_rows', probs.data_ptr(), probs.shape[1], tab['n_p'], tab['p_p'], u.ctypes.data, 8, head1.ctypes.data, tie.ctypes.data)
            out[1] = _nucleus_with_draw(probs.numpy()[1, :tab['n'][1]], self.SAMPLE_P[1], u[1]) if tie[0] >> 1 & 1 else head1[1]
        return torch.from_numpy(out.astype(np.int64))

    def sample(self, x, index):
        t, p = self.SAMPLE_T, self.SAMPLE_P
        return torch.tensor([sampling(x[j][:, index, :], p[j], t[j]) for j in range(8)])


# ---------------------------------------------------------------------------------------------------------------------
# Fine-tune heads. Same constructor arguments, attribute names and state_dict keys as the reference
# (model.py:128-272); the nn.Linear / nn.Sequential members are parameter holders, the arithmetic runs through the HIP ops of
# heads.py (exact f32 on top of the backbone's hidden states).
class SelfAttention(nn.Module):
    """model.py:128-143: r-aspect attention pooling weights, softmax over the sequence axis."""

    def __init__(self, input_dim, da, r):
        super().__init__()
        self.ws1 = nn.Linear(input_dim, da, bias=False)
        self.ws2 = nn.Linear(da, r, bias=False)

    def scores(self, h):
        """softmax(ws2(tanh(ws1(h))), dim=1): (B, S, r), i.e. attn_mat before the reference's permute(0, 2, 1)."""
        from . import heads
        return heads.softmax_dim1(heads.linear(heads.act(heads.linear(h, self.ws1.weight), 'tanh'), self.ws2.weight))

    def forward(self, h):
        return self.scores(h).permute(0, 2, 1)


class SequenceClassification(nn.Module):
    """model.py:165-218: the backbone is run with decoder input = encoder input (model.py:203), attention-pooled into r = 4
    aspects, flattened and classified by Dropout(0.1) -> Linear(hs r, 256) -> ReLU -> Linear(256, class_num)."""

    def __init__(self, pianobart, class_num, hs, da=128, r=4):
        super().__init__()
        self.pianobart = pianobart
        self.attention = SelfAttention(hs, da, r)
        self.classifier = nn.Sequential(nn.Dropout(0.1), nn.Linear(hs * r, 256), nn.ReLU(), nn.Linear(256, class_num))

    def forward(self, input_ids_encoder, encoder_attention_mask=None):
        from . import heads
        x = self.pianobart(input_ids_encoder=input_ids_encoder, input_ids_decoder=input_ids_encoder,
                           encoder_attention_mask=encoder_attention_mask, decoder_attention_mask=encoder_attention_mask).last_hidden_state
        m = heads.pool(self.attention.scores(x), x)                     # torch.bmm(attn_mat, x): (B, r, hs)
        flat = m.reshape(m.shape[0], -1)
        c = self.classifier
        y = heads.dropout(flat, c[0].p, self.training)
        y = heads.act(heads.linear(y, c[1].weight, c[1].bias), 'relu')
        return heads.linear(y, c[3].weight, c[3].bias)


class Excitation(nn.Module):
    """model.py:220-232 (squeeze-excitation gate; commented out of both classifiers in the reference, kept for API parity)."""

    def __init__(self, channel_dim, reduction=16):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(channel_dim, channel_dim // reduction), nn.ReLU(), nn.Linear(channel_dim // reduction, channel_dim), nn.Sigmoid())

    def forward(self, x):
        from . import heads
        y = heads.act(heads.linear(x, self.fc[0].weight, self.fc[0].bias), 'relu')
        y = heads.act(heads.linear(y, self.fc[2].weight, self.fc[2].bias), 'sigmoid')
        return heads.mul(x, y)


class TokenClassification(nn.Module):
    """model.py:236-272: per-token Dropout(0.1) -> Linear(hs, 256) -> ReLU -> Linear(256, class_num) on the decoder's hidden states.
    class_num >= 5 (the velocity task) swaps the decoder's input embedding for a class-label embedding of width 64 and its own
    Linear(64, d) (PianoBart.change_decoder_embedding, model.py:242-245); input_ids_decoder is then (B, S) labels."""

    def __init__(self, pianobart, class_num, hs, d_model=64):
        super().__init__()
        self.pianobart = pianobart
        if class_num >= 5:
            new_embedding = Embeddings(n_token=class_num, d_model=d_model)
            new_linear = nn.Linear(d_model, pianobart.bartConfig.d_model)
            self.pianobart.change_decoder_embedding(new_embedding, new_linear)
        self.classifier = nn.Sequential(nn.Dropout(0.1), nn.Linear(hs, 256), nn.ReLU(), nn.Linear(256, class_num))

    def forward(self, input_ids_encoder, input_ids_decoder, encoder_attention_mask=None, decoder_attention_mask=None):
        from . import heads
        x = self.pianobart(input_ids_encoder, input_ids_decoder, encoder_attention_mask, decoder_attention_mask).last_hidden_state
        c = self.classifier
        y = heads.dropout(x, c[0].p, self.training)
        y = heads.act(heads.linear(y, c[1].weight, c[1].bias), 'relu')
        return heads.linear(y, c[3].weight, c[3].bias)

