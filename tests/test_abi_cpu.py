"""CPU: the C-ABI library builds, loads, and exports every symbol include/pianobart_hip.h declares.
No compute call is made here (no GPU in the build container)."""
import ctypes
import os

import pytest

from pianobart_amd import _lib


def test_header_parses_and_library_exports_all():
    decls = _lib.parse_header()
    assert len(decls) >= 20 and 'pb_gemm' in decls and 'pb_adamw_step' in decls
    if not os.path.exists(_lib.LIB_PATH):
        from pianobart_amd.build import build
        build(verbose=False)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in decls:
        assert hasattr(dll, name), 'library does not export %s' % name
    assert _lib.LIB.query('pb_abi_version') == 10
    assert _lib.LIB.query('pb_ln_partials_floats', 768) == 512 * 3 * 768


def test_gemm_desc_layout_matches_header():
    # 6 pointers + 10 int32 + 10 int64 + 2 floats + 2 int32 + 1 pointer + colsum out / ws + rowdot out / ld
    assert ctypes.sizeof(_lib.GemmDesc) == 6 * 8 + 10 * 4 + 10 * 8 + 2 * 4 + 2 * 4 + 8 + 2 * 8 + 2 * 8


def test_attn_desc_layout_matches_header():
    """_lib.AttnDesc is generated from the header's typedef: the compiler's size of pb_attn_desc and the number of its members."""
    assert ctypes.sizeof(_lib.AttnDesc) == _lib.LIB.query('pb_attn_desc_bytes')
    src = open(_lib.HEADER).read()
    body = src[src.index('typedef struct pb_attn_desc {'):src.index('} pb_attn_desc;')].split('{', 1)[1]
    assert len(_lib.AttnDesc._fields_) == sum(decl.count(',') + 1 for decl in body.split(';') if decl.strip()) == 47
    # 8-byte members first, then the 4-byte ones: no implicit padding anywhere
    assert ctypes.sizeof(_lib.AttnDesc) == sum(ctypes.sizeof(t) for _, t in _lib.AttnDesc._fields_)


def _attn_desc(dtype, **over):
    """A dense B = 2, H = 2, S = 192, head_dim 64 call over dummy (non-null, 16-byte aligned) addresses: only good for calls that are
    refused, or found empty, before any HIP call."""
    d = _lib.AttnDesc()
    for n in ('q', 'k', 'v', 'o', 'dout', 'dq', 'dk', 'dv', 'lse', 'delta'):
        setattr(d, n, 0x10000)
    for n in ('q', 'k', 'v', 'o', 'dq', 'dk', 'dv'):
        setattr(d, n + '_ss', 128)
        setattr(d, n + '_sb', 192 * 128)
    d.dtype, d.B, d.H, d.Sq, d.Sk, d.hd, d.flags, d.scale = dtype, 2, 2, 192, 192, 64, 0, 0.125
    for n, v in over.items():
        setattr(d, n, v)
    return d


_ROWS4 = dict(q_off=0x10000, q_len=0x10000, k_off=0x10000, k_len=0x10000)
_REFUSED = [  # (case, dtypes, descriptor fields, what the message must name)
    ('head_dim', 'both', dict(hd=48), 'head_dim 48'),
    ('row_stride', (_lib.PB_BF16,), dict(k_ss=4), 'k_ss = 4'),
    ('row_stride', (_lib.PB_F32X3,), dict(k_ss=2), 'k_ss = 2'),
    ('four_row_descriptors', 'both', _ROWS4, 'k_vis'),
    ('dbias_without_ws', 'both', dict(dbias_q=0x10000, dbias_k=0x10000, dbias_v=0x10000), 'dbias'),
    ('one_pass_hd128', 'both', dict(flags=_lib.ATTN_ONE_PASS, hd=128, dq_ws=0x10000), 'head_dim 128'),
    ('dbias_x3', (_lib.PB_F32X3,), dict(dbias_q=0x10000, dbias_k=0x10000, dbias_v=0x10000, dbias_ws=0x10000), 'dbias'),
]


@pytest.mark.parametrize('entry', ['pb_attn_fwd', 'pb_attn_bwd'])
@pytest.mark.parametrize('case,dtype,fields,names', [(c, dt, f, n) for c, dts, f, n in _REFUSED
                                                     for dt in ((_lib.PB_BF16, _lib.PB_F32X3) if dts == 'both' else dts)])
def test_attn_desc_preconditions_refuse_without_a_gpu(entry, case, dtype, fields, names):
    """Every precondition of pb_attn_fwd / pb_attn_bwd is checked before the first HIP call, and reads the descriptor at the offsets the
    binding writes: a bad value planted in one field comes back, by name or by value, in the error."""
    with pytest.raises(_lib.PBError) as e:
        _lib.LIB.call(entry, ctypes.byref(_attn_desc(dtype, **fields)), None)
    assert entry in str(e.value) and '(-2)' in str(e.value) and names in str(e.value), str(e.value)


@pytest.mark.parametrize('entry', ['pb_attn_fwd', 'pb_attn_bwd'])
@pytest.mark.parametrize('dtype', [_lib.PB_BF16, _lib.PB_F32X3])
def test_attn_desc_empty_batch_returns_ok(entry, dtype):
    _lib.LIB.call(entry, ctypes.byref(_attn_desc(dtype, B=0)), None)       # raises on any non-zero status


def test_ops_refuse_cpu_tensors():
    import torch
    from pianobart_amd import ops
    x = torch.zeros(4, 4)
    with pytest.raises(_lib.PBError):
        ops.gemm(x, x, x, M=4, N=4, K=4, dtype=_lib.PB_F32)


def test_persistent_gemm_isa_has_no_spills_and_no_copies_of_in_flight_fragments():
    """tools/check_gemm_isa.py on the cross-compiled gfx950 code: a spilled vector register would enter the K loop's counted vmcnt queue,
    and any instruction other than the transposed reads and the MFMAs naming v200-v247 inside the TN loop would touch data still in flight."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('check_gemm_isa', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'check_gemm_isa.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    errs, meta = mod.check(mod.disassemble())
    assert len(meta) == 2 and not errs, errs[:5]


def test_persistent_gemm_waits_for_exactly_what_its_epilogues_issue():
    """tools/check_gemm_epilogue_vmem.py: the persistent GEMM's cross-item wait (`pend`) is a hand count of the VMEM instructions each epilogue
    variant leaves in flight; the check compiles every variant alone (probe kernels over the textually included pb_gemm2.hip), counts its global loads and
    stores in the gfx950 ISA and compares with the `pend` literals of the kernel source -- one store more or fewer in an epilogue fails here instead of racing."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location('check_gemm_epilogue_vmem', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools', 'check_gemm_epilogue_vmem.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    errs, got, table = mod.check()
    assert len(got) == 7 and not errs, errs
    assert table == {'plain': 16, 'wide': 32, 'epf': 32, 'epf_cs': 36, 'epf3': 40}


def test_attention_wrappers_refuse_cpu_tensors():
    """Every tensor of an attention call goes through the same device check as the other ops: a host lse, mask or operand never
    reaches pb_attn_fwd / pb_attn_bwd as a device address."""
    import torch
    from pianobart_amd import ops
    B, H, S, hd = 1, 1, 64, 64
    x = torch.zeros(B * S, hd, dtype=torch.bfloat16)
    t = (x, 0, hd, S * hd)
    lse = torch.zeros(B, H, S)
    with pytest.raises(_lib.PBError, match='HIP device tensors'):
        ops.flash_fwd(t, t, t, t, lse, None, B, H, S, S, hd, 0.125, False)
    with pytest.raises(_lib.PBError, match='HIP device tensors'):
        ops.flash_bwd(t, t, t, t, x, lse, torch.ones(B, S), t, t, t, lse.clone(), B, H, S, S, hd, 0.125, False)
