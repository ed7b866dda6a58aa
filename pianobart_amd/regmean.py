"""python -m pianobart_amd.regmean: the RegMean weights (Gram matrices of every backbone linear layer's inputs) of ONE fine-tuned
classifier on its own training data, for
`python -m pianobart_amd.model_merge --method regmean_merging --regmean a.regmean.pt,b.regmean.pt`.

    python -m pianobart_amd.regmean --ckpt result/finetune/composer_x/model_best.ckpt --task composer --dataset Pianist8 \\
        --num_examples 256 --batch_size 8 --output composer.regmean.pt

The flags and the loading of the model and its training split are those of pianobart_amd.fisher (file order, not shuffled). Written:
{'regmean': {Linear weight name: (K, K) f32 tensor}, 'num_rows': the divisor, 'num_examples': the examples counted, 'task': ..,
'precision': ..}. Names that read the same input (q / k / v; every decoder layer's cross-attention k / v) hold one tensor, stored once.
encoder_linear.weight has no entry and is averaged by the merge."""
import torch

from .fisher import get_args_fisher, load_classifier

get_args_regmean = get_args_fisher                           # the same flags, defaults and checks


def regmean(argv=None):
    args = get_args_regmean(argv)
    from .merge import regmean_pass
    model, loader, seq, device = load_classifier(args)
    weights, num_rows, num_counted = regmean_pass(model, loader, args.num_examples, seq, device)
    host = {}                                                # one CPU copy per matrix: shared entries stay shared in the file
    for v in weights.values():
        if id(v) not in host:
            host[id(v)] = v.detach().cpu().clone()
    torch.save({'regmean': {k: host[id(v)] for k, v in weights.items()}, 'num_rows': num_rows, 'num_examples': num_counted, 'task': args.task,
                'precision': args.precision}, args.output)
    print('   [regmean] %s: %d matrices for %d weights over %d rows of %d examples -> %s' % (args.ckpt, len(host), len(weights), num_rows, num_counted,
                                                                                          args.output))
    return weights


if __name__ == '__main__':
    regmean()
