"""python -m pianobart_amd.model_merge: merge fine-tuned PianoBart backbones into one checkpoint (the reference's model_merge.py).

The reference's flags keep their names and defaults; its script hard-codes mask_merging, here `--method` chooses (same default).
`--method fisher_merging --fisher a.fisher.pt,b.fisher.pt` weights every model by the Fisher weights `python -m pianobart_amd.fisher` wrote for it;
`--method regmean_merging --regmean a.regmean.pt,b.regmean.pt [--reduce_non_diagonal_ratio 0.9]` solves every linear layer's least-squares
problem from the Gram matrices `python -m pianobart_amd.regmean` wrote for each model.
Checkpoints are read as this project's trainers write them ({'state_dict': ...} or a bare dict, `module.` / `pianobart.` prefixes
stripped, head parameters dropped with a message, a file without any backbone key refused), merged on the device by
pianobart_amd.merge, and written as {'state_dict': ...}: what PianoBart.load_state_dict and every trainer's --ckpt read."""
import argparse

import torch

from ._lib import PBError
from .merge import METHODS, MergePlan, backbone_state_dict, merge_state_dicts


def get_args_merge(argv=None):
    parser = argparse.ArgumentParser(description='')

    parser.add_argument('--dict_file', type=str, default='./Data/Octuple.pkl')

    parser.add_argument('--pretrain_ckpt', type=str, default='./pianobart.ckpt')
    parser.add_argument('--model_path', type=str, default='')  # split by ','
    parser.add_argument('--output_path', type=str, default='./merge_pianobart.pth')

    parser.add_argument('--max_seq_len', type=int, default=1024, help='all sequences are padded to `max_seq_len`')
    parser.add_argument('--hs', type=int, default=1024)
    parser.add_argument('--layers', type=int, default=8)
    parser.add_argument('--ffn_dims', type=int, default=2048)
    parser.add_argument('--heads', type=int, default=8)

    parser.add_argument('--mask_apply_method', type=str, default="average_merging")
    parser.add_argument('--mask_strategy', type=str, default="random")
    parser.add_argument('--use_weight_rescale', action='store_false')  # True unless given, as in the reference
    parser.add_argument('--weight_format', type=str, default="delta_weight")
    parser.add_argument('--weight_mask_rate', type=float, default=0.8)

    # ours
    parser.add_argument('--method', type=str, default='mask_merging', help=' | '.join(METHODS))
    parser.add_argument('--scaling_coefficient', type=float, default=1.0)
    parser.add_argument('--param_value_mask_rate', type=float, default=0.8, help='TIES: share of the smallest-magnitude task-vector entries trimmed')
    parser.add_argument('--weight_mask_rates', type=str, default='', help='r1,r2,..: one mask rate per model (default: --weight_mask_rate for all)')
    parser.add_argument('--seed', type=int, default=0, help='seed of the random masks')
    parser.add_argument('--exclude', action='append', default=[], metavar='REGEX', help='parameter names (re.match) kept from the pre-trained model')
    # --method fisher_merging (absent from the namespace unless given: see fisher_kwargs for the defaults)
    S = argparse.SUPPRESS
    parser.add_argument('--fisher', type=str, default=S, help='a.fisher.pt,b.fisher.pt: one file of pianobart_amd.fisher per model of --model_path, in its order')
    parser.add_argument('--fisher_scaling_coefficients', type=str, default=S, help='c1,c2,..: one positive coefficient per model (default: 1/N each)')
    parser.add_argument('--no_normalize_fisher_weight', action='store_true', default=S, help="do not scale each model by 1 / its Fisher weights' L2 norm")
    parser.add_argument('--minimal_fisher_weight', type=float, default=S, help='added to every Fisher weight (default 1e-6)')
    # --method regmean_merging (absent from the namespace unless given, as above)
    parser.add_argument('--regmean', type=str, default=S, help='a.regmean.pt,b.regmean.pt: one file of pianobart_amd.regmean per model of --model_path, in its order')
    parser.add_argument('--reduce_non_diagonal_ratio', type=float, default=S, help='off-diagonal Gram entries are multiplied by this (default 1.0)')
    return parser.parse_args(argv)


def plan_kwargs(args):
    rates = [float(r) for r in args.weight_mask_rates.split(',')] if args.weight_mask_rates else None
    return dict(method=args.method, mask_apply_method=args.mask_apply_method, mask_strategy=args.mask_strategy,
                use_weight_rescale=args.use_weight_rescale, weight_format=args.weight_format, weight_mask_rate=args.weight_mask_rate,
                weight_mask_rates=rates, scaling_coefficient=args.scaling_coefficient, param_value_mask_rate=args.param_value_mask_rate,
                seed=args.seed, exclude=args.exclude)


def fisher_kwargs(args):
    """(the Fisher files, the Fisher keyword arguments of MergePlan without the weights themselves); the reference's defaults."""
    files = [p for p in getattr(args, 'fisher', '').split(',') if p]
    coef = getattr(args, 'fisher_scaling_coefficients', '')
    return files, dict(fisher_scaling_coefficients=[float(c) for c in coef.split(',')] if coef else None,
                       normalize_fisher_weight=not getattr(args, 'no_normalize_fisher_weight', False),
                       minimal_fisher_weight=getattr(args, 'minimal_fisher_weight', 1e-6))


def load_fisher_file(path):
    f = torch.load(path, map_location='cpu', weights_only=False)
    if not isinstance(f, dict) or not isinstance(f.get('fisher'), dict):
        raise PBError("%s is not a file of pianobart_amd.fisher ({'fisher': {name: tensor}, ..})" % path)
    print('   [merge] %s: Fisher weights of %d tensors over %s examples (%s, %s)' % (path, len(f['fisher']), f.get('num_computed'), f.get('task'), f.get('precision')))
    return f['fisher']


def load_regmean_file(path):
    f = torch.load(path, map_location='cpu', weights_only=False)
    if not isinstance(f, dict) or not isinstance(f.get('regmean'), dict):
        raise PBError("%s is not a file of pianobart_amd.regmean ({'regmean': {name: tensor}, ..})" % path)
    print('   [merge] %s: Gram matrices for %d weights over %s rows of %s examples (%s, %s)' % (path, len(f['regmean']), f.get('num_rows'), f.get('num_examples'),
                                                                                              f.get('task'), f.get('precision')))
    return f['regmean']


def model_merge(argv=None):
    args = get_args_merge(argv)
    paths = [p for p in args.model_path.split(',') if p]
    kw = plan_kwargs(args)
    fisher_files = []
    if args.method == 'fisher_merging':
        fisher_files, fkw = fisher_kwargs(args)
        kw.update(fkw, fisher_weights=fisher_files or None)         # the file names stand in for the weights until they are read
    regmean_files = []
    if args.method == 'regmean_merging':
        regmean_files = [p for p in getattr(args, 'regmean', '').split(',') if p]
        kw.update(regmean_weights=regmean_files or None, reduce_non_diagonal_ratio=getattr(args, 'reduce_non_diagonal_ratio', 1.0))
    MergePlan(len(paths), **kw)                                     # every refusal that needs no file comes first

    from .model import BartConfig, PianoBart
    from .pretrain import _load_vocab
    print("Loading Dictionary")
    e2w, w2e = _load_vocab(args.dict_file)
    configuration = BartConfig(max_position_embeddings=args.max_seq_len, d_model=args.hs, encoder_layers=args.layers, encoder_ffn_dim=args.ffn_dims,
                               encoder_attention_heads=args.heads, decoder_layers=args.layers, decoder_ffn_dim=args.ffn_dims,
                               decoder_attention_heads=args.heads)
    pianobart = PianoBart(bartConfig=configuration, e2w=e2w, w2e=w2e)
    own = pianobart.state_dict()

    def load(path, label):
        sd = backbone_state_dict(torch.load(path, map_location='cpu', weights_only=False), own, label)
        for k, v in sd.items():
            if tuple(v.shape) != tuple(own[k].shape):
                raise PBError('%s: %s is %s, the model of the flags holds %s' % (label, k, tuple(v.shape), tuple(own[k].shape)))
        return sd

    pre = load(args.pretrain_ckpt, args.pretrain_ckpt)
    missing = [k for k in own if k not in pre]
    if missing:
        raise PBError('%s lacks %d backbone keys (first: %s): a pre-trained checkpoint must be complete' % (args.pretrain_ckpt, len(missing), missing[0]))
    pianobart.load_state_dict(pre, strict=True)
    pre = pianobart.state_dict()                                    # tied tables share storage again: one parameter, as in named_parameters()
    print(paths)
    models = []
    for p in paths:
        print("Load From " + p)
        sd = load(p, p)
        missing = [k for k in pre if k not in sd]
        if missing:
            raise PBError('%s lacks %d backbone keys (first: %s)' % (p, len(missing), missing[0]))
        models.append(sd)
    if fisher_files:
        kw['fisher_weights'] = [load_fisher_file(p) for p in fisher_files]
    if regmean_files:
        kw['regmean_weights'] = [load_regmean_file(p) for p in regmean_files]
    merged = merge_state_dicts(pre, models, **kw)
    pianobart.load_state_dict(merged, strict=True)
    torch.save({'state_dict': pianobart.state_dict()}, args.output_path)
    print('   [merge] %s of %d models -> %s' % (args.method, len(models), args.output_path))


if __name__ == '__main__':
    model_merge()
