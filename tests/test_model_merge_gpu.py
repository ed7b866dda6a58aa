"""GPU: python -m pianobart_amd.model_merge end to end on a tiny backbone -- checkpoints as the trainers write them (a {'state_dict': ...}
file, a bare dict with `module.pianobart.` prefixes and head parameters), the merged file equals merge_state_dicts on the same state dicts
byte for byte, loads into PianoBart with strict=True, and reads like every trainer's --ckpt ({'state_dict': ...})."""
import copy
import json
import os

import pytest
import torch

gpu = pytest.mark.gpu


@gpu
def test_model_merge_command_line(tmp_path, capsys):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from pianobart_amd._lib import PBError
    from pianobart_amd.merge import merge_state_dicts
    from pianobart_amd.model import BartConfig, PianoBart
    from pianobart_amd.model_merge import model_merge
    from tests.golden_util import load_vocab, randomize_params
    e2w, w2e = load_vocab()
    dict_file = str(tmp_path / 'dict.json')
    with open(dict_file, 'w') as f:
        json.dump({'e2w': e2w}, f)
    shape = dict(max_seq_len=32, hs=64, layers=1, ffn_dims=128, heads=4)
    cfg = BartConfig(max_position_embeddings=32, d_model=64, encoder_layers=1, decoder_layers=1, encoder_ffn_dim=128, decoder_ffn_dim=128,
                     encoder_attention_heads=4, decoder_attention_heads=4)
    pre = PianoBart(cfg, e2w, w2e)
    randomize_params(pre, 5)
    g = torch.Generator().manual_seed(6)
    fts = []
    for i in range(2):
        m = copy.deepcopy(pre)
        with torch.no_grad():
            for q in m.parameters():
                q.add_(torch.randn(q.shape, generator=g) * 0.01)
        fts.append(m)
    torch.save({'state_dict': pre.state_dict(), 'epoch': 1}, str(tmp_path / 'pre.ckpt'))
    wrapped = {'module.pianobart.' + k: v for k, v in fts[0].state_dict().items()}
    wrapped['module.classifier.weight'] = torch.zeros(3, 64)
    torch.save(wrapped, str(tmp_path / 'a.ckpt'))
    torch.save({'state_dict': {'pianobart.' + k: v for k, v in fts[1].state_dict().items()}}, str(tmp_path / 'b.ckpt'))
    torch.save({'state_dict': {'classifier.weight': torch.zeros(3, 64)}}, str(tmp_path / 'heads_only.ckpt'))
    flags = ['--dict_file', dict_file, '--pretrain_ckpt', str(tmp_path / 'pre.ckpt')] + [x for k, v in shape.items() for x in ('--' + k, str(v))]
    out = str(tmp_path / 'merged.ckpt')
    model_merge(flags + ['--model_path', '%s,%s' % (tmp_path / 'a.ckpt', tmp_path / 'b.ckpt'), '--output_path', out, '--method', 'ties_merging',
                         '--scaling_coefficient', '0.9'])
    said = capsys.readouterr().out
    assert "stripping the 'module.' prefix" in said and 'dropped 1 keys' in said and 'backbone keys matched' in said
    merged = torch.load(out, map_location='cpu', weights_only=False)['state_dict']
    want = merge_state_dicts(pre.state_dict(), [f.state_dict() for f in fts], method='ties_merging', scaling_coefficient=0.9)
    assert list(merged) == list(pre.state_dict())
    for k in want:
        assert merged[k].numpy().tobytes() == want[k].numpy().tobytes(), k
    assert any(not torch.equal(merged[k], pre.state_dict()[k]) for k in merged)
    PianoBart(cfg, e2w, w2e).load_state_dict(merged, strict=True)
    with pytest.raises(PBError, match='none of its 1 keys'):
        model_merge(flags + ['--model_path', '%s,%s' % (tmp_path / 'a.ckpt', tmp_path / 'heads_only.ckpt'), '--output_path', out])
    with pytest.raises(PBError, match='at least two'):
        model_merge(flags + ['--model_path', str(tmp_path / 'a.ckpt'), '--output_path', out])
    with pytest.raises(PBError, match='fisher_merging'):
        model_merge(flags + ['--model_path', 'x,y', '--method', 'fisher_merging'])
