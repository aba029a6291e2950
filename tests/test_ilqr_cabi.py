"""The C ABI of the feedback rollout and the LQ backward pass (include/diygym_hip.h): declared, typed by the binding, exported,
refusing a NULL world without touching a device; the named tuples' fields in the entries' order; and the LDS the backward kernel asks for
fits every body it takes (the feedback rollout's workspace is fdq_slots(n), which tests/test_fd_cabi.py proves every scene has).  Runs without a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'libdiygym_hip.so')
DG_ERR_ARG = -4
vp, i32, f32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_float, ctypes.c_double
ENTRIES = {
    'dg_world_rollout_feedback': (['dg_world* w', 'const float* state', 'int32_t body', 'int32_t frame', 'const float* local_pos', 'int32_t K', 'int32_t T', 'float dt',
                                   'int32_t joint_damping', 'const float* q0', 'const float* qd0', 'const float* tau_ff', 'const float* dtau', 'const float* alpha',
                                   'const float* gain', 'const float* q_ref', 'const float* qd_ref', 'const float* tau_limit', 'float* q_out', 'float* qd_out',
                                   'float* tau_out', 'float* pos_out', 'int32_t* singular', 'void* stream'],
                                  [vp, vp, i32, i32, ctypes.POINTER(f32), i32, i32, f32, i32] + [vp] * 15),
    'dg_world_lq_backward': (['dg_world* w', 'int32_t body', 'int32_t T', 'int32_t P', 'int32_t PC', 'int32_t substeps', 'double dt', 'const float* A_q', 'const float* A_v',
                              'const float* Minv', 'const float* lxx', 'const float* luu', 'const float* lx', 'const float* lu', 'const float* lxx_T', 'const float* lx_T',
                              'const float* mu', 'float* K_out', 'float* k_out', 'float* dV', 'int32_t* status', 'void* stream'],
                             [vp, i32, i32, i32, i32, i32, f64] + [vp] * 15),
}


@pytest.mark.parametrize('name', sorted(ENTRIES))
def test_header_declares_the_entry_and_the_binding_types_it(name):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'diygym_hip.h')).read(), flags=re.S)
    decl = re.search(r'\bint32_t\s+%s\s*\(([^)]*)\)\s*;' % name, text)
    assert decl, name
    assert [' '.join(p.split()) for p in decl.group(1).split(',')] == ENTRIES[name][0]
    from diy_gym_amd import backend
    res, argtypes = backend.SYMBOLS[name]
    assert res is i32 and argtypes == ENTRIES[name][1]
    # the outputs, in the entries' order
    assert backend.FeedbackRollout._fields == ('q', 'qd', 'tau', 'pos', 'singular')
    assert backend.LqBackward._fields == ('K', 'k', 'dV', 'status')
    outs = [p.split()[-1] for p in ENTRIES[name][0] if p.startswith(('float*', 'int32_t*'))]
    assert outs == {'dg_world_rollout_feedback': ['q_out', 'qd_out', 'tau_out', 'pos_out', 'singular'], 'dg_world_lq_backward': ['K_out', 'k_out', 'dV', 'status']}[name]


def test_library_exports_them_and_they_refuse_a_null_world():
    lib = ctypes.CDLL(LIB)
    lib.dg_last_error.restype = ctypes.c_char_p
    for name, (_, argtypes) in ENTRIES.items():
        fn = getattr(lib, name)   # AttributeError: not exported
        fn.restype, fn.argtypes = i32, argtypes
    lp = (f32 * 3)(0.0, 0.0, 0.0)
    assert lib.dg_world_rollout_feedback(None, None, 0, 0, lp, 1, 1, 0.01, 0, *[None] * 15) == DG_ERR_ARG
    assert lib.dg_last_error() == b'dg_world_rollout_feedback: null argument'
    assert lib.dg_world_lq_backward(None, 0, 1, 1, 1, 1, 0.01, *[None] * 15) == DG_ERR_ARG
    assert lib.dg_last_error() == b'dg_world_lq_backward: null argument'


def test_the_backward_kernels_lds_fits_every_body_it_takes():
    """``lq_lds_doubles(n)`` as diy_gym_amd/csrc/dg_lqr.h defines it, evaluated here (as tests/test_fd_cabi.py evaluates fdq_slots): the
    figures of DESIGN's table, and below the 64 KiB a kernel gets without asking for more at the largest body the entry takes."""
    text = open(os.path.join(ROOT, 'diy_gym_amd', 'csrc', 'dg_lqr.h')).read()
    body = re.search(r'constexpr int lq_lds_doubles\(int n\)\s*\{\s*return ([^;]*);\s*\}', text).group(1)
    assert re.fullmatch(r'[\w\s+*()]+', body), body
    most = int(re.search(r'constexpr int LQ_MAX_JOINTS\s*=\s*(\d+)\s*;', text).group(1))
    lds = lambda n: 8 * eval(body, {'__builtins__': {}}, {'n': n})
    assert most == 12 and [lds(n) for n in (1, 3, 6, 12)] == [296, 2232, 8496, 33120] and lds(most) <= 64 * 1024
