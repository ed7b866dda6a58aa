"""python -m pianobart_amd.fisher: the Fisher weights of ONE fine-tuned classifier on its own training data, for
`python -m pianobart_amd.model_merge --method fisher_merging --fisher a.fisher.pt,b.fisher.pt`.

    python -m pianobart_amd.fisher --ckpt result/finetune/composer_x/model_best.ckpt --task composer --dataset Pianist8 \\
        --num_examples 256 --batch_size 8 --output composer.fisher.pt

The model-shape flags, --task / --dataset / --dataroot / --dict_file / --class_num / --precision are those of pianobart_amd.finetune. The
training split is read in file order (not shuffled): the first batches of the file are the examples used. Written:
{'fisher': {backbone parameter name: f32 tensor}, 'num_computed': the divisor, 'task': .., 'precision': ..}."""
import argparse

import torch

from ._lib import PBError


def pass_parser():
    """The flags a data pass over one fine-tuned classifier takes (this tool and pianobart_amd.regmean)."""
    parser = argparse.ArgumentParser(description='')
    parser.add_argument('--task', choices=['melody', 'velocity', 'composer', 'emotion'], required=True)
    parser.add_argument('--dataset', type=str, choices=('asap', 'Pianist8', 'POP909', 'EMOPIA', 'GiantMIDI1k'), required=True)
    parser.add_argument('--dataroot', type=str, default=None)
    parser.add_argument('--dict_file', type=str, default='./Data/Octuple.pkl')
    parser.add_argument('--ckpt', type=str, required=True, help='a fine-tune checkpoint as FinetuneTrainer.save_checkpoint writes it')
    parser.add_argument('--output', type=str, required=True)
    parser.add_argument('--num_examples', type=int, default=256, help='the pass ends before a batch once this many examples are counted')
    parser.add_argument('--batch_size', type=int, default=8)
    parser.add_argument('--class_num', type=int, default=None)
    parser.add_argument('--max_seq_len', type=int, default=1024, help='all sequences are padded to `max_seq_len`')
    parser.add_argument('--hs', type=int, default=1024)
    parser.add_argument('--layers', type=int, default=8)
    parser.add_argument('--ffn_dims', type=int, default=2048)
    parser.add_argument('--heads', type=int, default=8)
    parser.add_argument('--cuda_device', type=int, default=0)
    parser.add_argument('--precision', choices=['bf16', 'fp32', 'bf16x3'], default='bf16', help='backbone arithmetic of the pass')
    return parser


def get_args_fisher(argv=None):
    args = pass_parser().parse_args(argv)
    if args.class_num is None:
        args.class_num = {'melody': 4, 'velocity': 7, 'composer': 8, 'emotion': 4}[args.task]
    if args.num_examples < 1 or args.batch_size < 1:
        raise PBError('--num_examples and --batch_size must be positive')
    return args


def load_classifier(args):
    """(the fine-tuned classifier of --ckpt, its training split as an unshuffled loader, seq: a sequence task, the device)."""
    from torch.utils.data import DataLoader
    from .finetune import FinetuneDataset, load_data_finetune
    from .model import BartConfig, PianoBart, SequenceClassification, TokenClassification, checkpoint_state_dict
    from .pretrain import _load_vocab
    if not torch.cuda.is_available():
        raise PBError('pianobart_amd has no CPU execution path')
    device = torch.device('cuda', args.cuda_device)
    torch.cuda.set_device(device)
    e2w, w2e = _load_vocab(args.dict_file)
    X_train, _, _, y_train, _, _ = load_data_finetune(args.dataset, args.task, args.dataroot)
    loader = DataLoader(FinetuneDataset(X=X_train, y=y_train), batch_size=args.batch_size, shuffle=False)
    shape = dict(max_position_embeddings=args.max_seq_len, d_model=args.hs)
    for side in ('encoder', 'decoder'):
        shape.update({side + '_layers': args.layers, side + '_ffn_dim': args.ffn_dims, side + '_attention_heads': args.heads})
    pianobart = PianoBart(bartConfig=BartConfig(**shape), e2w=e2w, w2e=w2e, precision=args.precision)
    seq = args.task in ('composer', 'emotion')
    model = SequenceClassification(pianobart, args.class_num, args.hs) if seq else TokenClassification(pianobart, args.class_num + 1, args.hs)
    sd = torch.load(args.ckpt, map_location='cpu', weights_only=False)
    model.load_state_dict(checkpoint_state_dict(sd['state_dict'] if isinstance(sd, dict) and 'state_dict' in sd else sd), strict=True)
    return model, loader, seq, device


def fisher(argv=None):
    args = get_args_fisher(argv)
    from .merge import fisher_pass
    model, loader, seq, device = load_classifier(args)
    weights, num_computed = fisher_pass(model, loader, args.num_examples, args.batch_size, seq, device)
    torch.save({'fisher': {k: v.detach().cpu().clone() for k, v in weights.items()}, 'num_computed': num_computed, 'task': args.task,
                'precision': args.precision}, args.output)
    print('   [fisher] %s: %d tensors over %d examples counted -> %s' % (args.ckpt, len(weights), num_computed, args.output))
    return weights


if __name__ == '__main__':
    fisher()
