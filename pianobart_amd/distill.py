"""Knowledge distillation for the two language-model trainers (pretrain, finetune_generation): a small student is trained on a large
teacher's per-head distributions. The arithmetic lives in csrc/pb_distill.hip (one fused kernel between the head GEMM and its backward);
Engine.loss_and_grads(distill=..., smooth=...) wires it in; this module is the host side: the shared command-line arguments, loading a
teacher checkpoint, and the log columns. DESIGN.md 5 "Distillation" has the formulas and what is out of scope.

The teacher is frozen: eval mode, no gradient, no optimizer state, no reducer; it is not part of the student's checkpoint. Under data
parallelism every rank loads its own copy. It reads the batch the student reads (augmented and corrupted)."""
import torch

from ._lib import PBError
from .model import BartConfig, PianoBart, PianoBartLM, checkpoint_state_dict


class Distill:
    """What Engine.loss_and_grads(distill=...) takes: .teacher (the teacher's Engine), .alpha (weight of the soft part, 0 .. 1) and .tau
    (temperature > 0). Holds the teacher model so that it lives as long as the plan."""

    def __init__(self, model, alpha=0.5, tau=2.0):
        alpha, tau = float(alpha), float(tau)
        if not 0.0 <= alpha <= 1.0:
            raise PBError('--distill_alpha must lie in [0, 1] (got %r)' % alpha)
        if not 0.0 < tau < float('inf'):
            raise PBError('--distill_temperature must be finite and > 0 (got %r)' % tau)
        self.model, self.alpha, self.tau = model, alpha, tau

    @property
    def teacher(self):
        return self.model._get_engine()


def add_arguments(parser):
    """The distillation / label-smoothing flags of pretrain and finetune_generation (off unless --distill_from / --label_smoothing is given)."""
    parser.add_argument('--distill_from', type=str, default=None, metavar='CKPT',
                        help='train on the logits of this teacher: a finetune_generation checkpoint or a pre-train checkpoint written by this '
                             'project (not in the reference; off by default)')
    parser.add_argument('--teacher_hs', type=int, default=1024, help='teacher d_model')
    parser.add_argument('--teacher_layers', type=int, default=8, help='teacher encoder / decoder layers')
    parser.add_argument('--teacher_ffn_dims', type=int, default=2048, help='teacher FFN width')
    parser.add_argument('--teacher_heads', type=int, default=8, help='teacher attention heads')
    parser.add_argument('--teacher_precision', type=str, default='bf16', choices=['bf16', 'fp32', 'bf16x3'], help='teacher arithmetic')
    parser.add_argument('--distill_alpha', type=float, default=0.5, help='weight of the soft part: loss = (1 - alpha) CE + alpha T^2 KL')
    parser.add_argument('--distill_temperature', type=float, default=2.0, help='temperature T of the teacher and student distributions in the KL')
    parser.add_argument('--label_smoothing', type=float, default=0.0, help='label smoothing eps of the hard part, in [0, 1)')


def check_smoothing(eps):
    eps = float(eps)
    if not 0.0 <= eps < 1.0:
        raise PBError('--label_smoothing must lie in [0, 1) (got %r)' % eps)
    return eps


def _window(sd, prefix):
    w = sd.get(prefix + 'bart.encoder.embed_positions.weight')
    return None if w is None else int(w.shape[0]) - 2


def load_teacher(path, e2w, w2e, hs=1024, layers=8, ffn_dims=2048, heads=8, precision='bf16', device=None):
    """A frozen PianoBartLM from a checkpoint WITH language-model heads:
      * a finetune_generation checkpoint: 'state_dict' is the whole model ('pianobart.*' and 'mask_lm.*');
      * a pre-train checkpoint this project wrote (Pretrainer.save_checkpoint): 'state_dict' is PianoBart alone and the heads travel under
        'optimizer' -> 'mask_lm'.
    A file without heads (a pre-train checkpoint of the reference holds PianoBart alone) is refused by name: there are no logits to distill.
    The window (max_position_embeddings) is the file's own. Returns the model in eval mode with requires_grad off, on `device` if given."""
    ck = torch.load(path, map_location='cpu', weights_only=False)
    if not isinstance(ck, dict) or 'state_dict' not in ck:
        raise PBError("%s is not a checkpoint of the trainers (no 'state_dict')" % path)
    sd = checkpoint_state_dict(ck['state_dict'])
    opt = ck.get('optimizer')
    whole = any(k.startswith('mask_lm.') for k in sd)
    heads_sd = opt.get('mask_lm') if isinstance(opt, dict) else None
    if not whole and heads_sd is None:
        raise PBError('%s has no LM heads (a pre-train checkpoint of the reference holds PianoBart alone; this project keeps the heads under '
                      "optimizer['mask_lm']): there are no logits to distill" % path)
    window = _window(sd, 'pianobart.' if whole else '')
    if window is None:
        raise PBError('%s: the state_dict holds no %sbart.encoder.embed_positions.weight: not a PianoBart checkpoint' % (path, 'pianobart.' if whole else ''))
    cfg = BartConfig(max_position_embeddings=window, d_model=hs, encoder_layers=layers, decoder_layers=layers, encoder_ffn_dim=ffn_dims,
                     decoder_ffn_dim=ffn_dims, encoder_attention_heads=heads, decoder_attention_heads=heads)
    model = PianoBartLM(PianoBart(bartConfig=cfg, e2w=e2w, w2e=w2e, precision=precision))
    try:
        if whole:
            model.load_state_dict(sd, strict=True)
        else:
            model.pianobart.load_state_dict(sd, strict=True)
            model.mask_lm.load_state_dict(heads_sd, strict=True)
    except RuntimeError as err:
        raise PBError('%s does not fit a teacher of --teacher_hs %d --teacher_layers %d --teacher_ffn_dims %d --teacher_heads %d: %s'
                      % (path, hs, layers, ffn_dims, heads, str(err)[:400]))
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model.to(device) if device is not None else model


def from_args(args, e2w, w2e, device=None):
    """(Distill or None, label-smoothing eps) of a driver's arguments."""
    eps = check_smoothing(getattr(args, 'label_smoothing', 0.0))
    if not getattr(args, 'distill_from', None):
        return None, eps
    plan = Distill(None, args.distill_alpha, args.distill_temperature)          # the scalars are checked before the file is read
    plan.model = load_teacher(args.distill_from, e2w, w2e, args.teacher_hs, args.teacher_layers, args.teacher_ffn_dims, args.teacher_heads,
                              args.teacher_precision, device)
    return plan, eps


def step_kwargs(plan, eps):
    """The keyword arguments of Engine.loss_and_grads for a TRAINING step (validation stays plain cross-entropy): empty when nothing is on."""
    kw = {}
    if plan is not None:
        kw['distill'] = plan
    if eps:
        kw['smooth'] = eps
    return kw


def progress_suffix(extra, counts, weights):
    """What a training 'Loss:' line gains behind its existing columns: the hard cross-entropy and the KL term of the step, each the mean
    over the heads weighted as the line's total loss is (extra: the 16 sums of Engine.last_distill_sums, counts: the 8 mask counts)."""
    import numpy as np
    w = np.asarray(weights, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        hard, kl = np.asarray(extra[0:8], dtype=np.float64) / counts, np.asarray(extra[8:16], dtype=np.float64) / counts
    return ' | hard: {:06f} | kl: {:06f}'.format(float((hard * w).sum() / w.sum()), float((kl * w).sum() / w.sum()))
