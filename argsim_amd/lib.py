"""ctypes binding of libargsim_vae.so (include/argsim_vae.h).

The library is the product; there is NO CPU fallback.  If the shared object is missing or no
HIP device is present, the functions here raise."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libargsim_vae.so')
CSRC = os.path.join(_HERE, 'csrc')


def source_digest():
    """sha1 over the kernel and host sources the library is built from (csrc/*.hip, *.cpp, *.h and the C-ABI header): names a
    build.  The committed rocprofv3 summaries under profiles/ record it (scripts/summarize_profile.py) and bench.py only quotes
    their counters for the SAME sources -- the GPU box has no .git to ask for a commit."""
    import glob
    import hashlib
    h = hashlib.sha1()
    files = sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.cpp')) + glob.glob(os.path.join(CSRC, '*.h')))
    files.append(os.path.join(os.path.dirname(_HERE), 'include', 'argsim_vae.h'))
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


class AvaeConfig(C.Structure):
    _fields_ = [('dim_tgt', C.c_int32), ('dim_emb', C.c_int32), ('dim_rep', C.c_int32), ('rnn_layers', C.c_int32),
                ('accelerate', C.c_float), ('learn_rate', C.c_float), ('bos', C.c_int32), ('eos', C.c_int32),
                ('max_batch', C.c_int32), ('max_len', C.c_int32), ('kl_beta', C.c_float), ('free_bits', C.c_float),
                ('compute_dtype', C.c_int32)]


GRAD_HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int64, C.c_int64)

class AvaeSampleConfig(C.Structure):
    _fields_ = [('temperature', C.c_float), ('top_k', C.c_int32), ('seed', C.c_uint64)]


class AvaeSamplePConfig(C.Structure):
    _fields_ = [('temperature', C.c_float), ('top_k', C.c_int32), ('seed', C.c_uint64), ('top_p', C.c_float), ('reserved', C.c_int32)]


class AvaeBeamConfig(C.Structure):
    _fields_ = [('width', C.c_int32), ('length_alpha', C.c_float)]


class AvaeScoreConfig(C.Structure):
    _fields_ = [('k', C.c_int32), ('seed', C.c_uint64)]


class AvaeKnnConfig(C.Structure):
    _fields_ = [('k', C.c_int32), ('metric', C.c_int32), ('idx_base', C.c_int64), ('self_base', C.c_int64), ('carry', C.c_int32),
                ('reserved', C.c_int32)]


class AvaeAggConfig(C.Structure):
    _fields_ = [('self_base', C.c_int64), ('reserved', C.c_int32 * 2)]


class AvaeProbeConfig(C.Structure):
    _fields_ = [('max_newton', C.c_int32), ('max_cg', C.c_int32), ('tol', C.c_float), ('reserved', C.c_int32)]


class AvaeProbeL1Config(C.Structure):
    _fields_ = [('max_newton', C.c_int32), ('max_inner', C.c_int32), ('tol', C.c_float), ('reserved', C.c_int32)]


class AvaeWardConfig(C.Structure):
    _fields_ = [('reserved', C.c_int32 * 2)]


class AvaeAffinityConfig(C.Structure):
    _fields_ = [('metric', C.c_int32), ('max_iter', C.c_int32), ('convergence_iter', C.c_int32), ('use_preference', C.c_int32),
                ('noise', C.c_int32), ('warm', C.c_int32), ('damping', C.c_float), ('preference', C.c_float), ('seed', C.c_uint64),
                ('reserved', C.c_int32 * 2)]


class AvaeTsneConfig(C.Structure):
    _fields_ = [('perplexity', C.c_double), ('early_exaggeration', C.c_double), ('min_grad_norm', C.c_double), ('learning_rate', C.c_float),
                ('max_iter', C.c_int32), ('it0', C.c_int32), ('exaggeration_iter', C.c_int32), ('n_iter_check', C.c_int32),
                ('n_iter_without_progress', C.c_int32), ('init', C.c_int32), ('warm', C.c_int32), ('seed', C.c_uint64),
                ('reserved', C.c_int32 * 2)]


class AvaeKmeansConfig(C.Structure):
    _fields_ = [('k', C.c_int32), ('n_init', C.c_int32), ('max_iter', C.c_int32), ('metric', C.c_int32), ('init', C.c_int32),
                ('reserved', C.c_int32), ('tol', C.c_double), ('seed', C.c_uint64)]

class AvaeGmmConfig(C.Structure):
    _fields_ = [('k', C.c_int32), ('n_init', C.c_int32), ('max_iter', C.c_int32), ('covariance', C.c_int32), ('init', C.c_int32),
                ('reserved', C.c_int32), ('tol', C.c_double), ('reg_covar', C.c_double)]


class AvaeSilhouetteConfig(C.Structure):
    _fields_ = [('metric', C.c_int32), ('L', C.c_int32), ('reserved', C.c_int32), ('reserved2', C.c_int32)]


class AvaeDbscanConfig(C.Structure):
    _fields_ = [('metric', C.c_int32), ('min_samples', C.c_int32), ('max_rounds', C.c_int32), ('reserved', C.c_int32), ('eps', C.c_double)]


class AvaePcaConfig(C.Structure):
    _fields_ = [('pad', C.c_int32), ('max_sweeps', C.c_int32), ('reserved', C.c_int32), ('reserved2', C.c_int32)]


class AvaeMmdConfig(C.Structure):
    _fields_ = [('kernel', C.c_int32), ('metric', C.c_int32), ('G', C.c_int32), ('P', C.c_int32), ('nbw', C.c_int32), ('reserved', C.c_int32),
                ('gamma', C.c_double * 8)]


_P = C.c_void_p
# name -> (restype, argtypes); exactly the declarations of include/argsim_vae.h
SIGNATURES = {
    'avae_create': (C.c_int, [C.POINTER(AvaeConfig), C.c_int, C.POINTER(_P)]),
    'avae_destroy': (None, [_P]),
    'avae_last_error': (C.c_char_p, [_P]),
    'avae_set_stream': (C.c_int, [_P, _P]),
    'avae_get_dims': (C.c_int, [_P] + [C.POINTER(C.c_int32)] * 4),
    'avae_state_numel': (C.c_int64, [_P]),
    'avae_bind_state': (C.c_int, [_P, _P, _P, _P, _P]),
    'avae_param_count': (C.c_int, [_P]),
    'avae_param_name': (C.c_char_p, [_P, C.c_int]),
    'avae_param_info': (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    'avae_get_tensor': (C.c_int, [_P, C.c_char_p, C.c_int, _P]),
    'avae_set_tensor': (C.c_int, [_P, C.c_char_p, C.c_int, _P]),
    'avae_get_step': (C.c_int, [_P, C.POINTER(C.c_int64)]),
    'avae_set_step': (C.c_int, [_P, C.c_int64]),
    'avae_get_schedule': (C.c_int, [_P, C.POINTER(C.c_float)]),
    'avae_forward_backward': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _P, _P, C.c_float, C.c_float]),
    'avae_adam_step': (C.c_int, [_P]),
    'avae_train_step': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, _P, _P]),
    'avae_get_losses': (C.c_int, [_P, C.POINTER(C.c_float)]),
    'avae_set_grad_hook': (C.c_int, [_P, GRAD_HOOK, _P]),
    'avae_eval': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, C.POINTER(C.c_int32)]),
    'avae_encode': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    'avae_decode_init': (C.c_int, [_P, _P, C.c_int32, _P]),
    'avae_decode_step': (C.c_int, [_P, _P, _P, C.c_int32, _P, _P]),
    'avae_decode_greedy': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.POINTER(C.c_int32)]),
    'avae_decode_sample': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(AvaeSampleConfig), _P, _P, C.POINTER(C.c_int32)]),
    'avae_decode_sample_p': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(AvaeSamplePConfig), _P, _P, _P, C.POINTER(C.c_int32)]),
    'avae_decode_beam': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(AvaeBeamConfig), _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_int32)]),
    'avae_score': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(AvaeScoreConfig), _P, _P, _P, _P, _P, _P]),
    'avae_score_z': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    'avae_knn': (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.POINTER(AvaeKnnConfig), _P, _P]),
    'avae_agg_logq': (C.c_int, [_P, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, C.POINTER(AvaeAggConfig), _P, _P]),
    'avae_latent_moments': (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P]),
    'avae_probe_fit': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.POINTER(AvaeProbeConfig), _P, _P]),
    'avae_probe_decision': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, _P]),
    'avae_probe_fit_l1': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.POINTER(AvaeProbeL1Config), _P, _P]),
    'avae_ward': (C.c_int, [_P, _P, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(AvaeWardConfig), _P, _P, _P]),
    'avae_ward_cut': (C.c_int, [_P, _P, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), _P]),
    'avae_affinity': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(AvaeAffinityConfig), _P, _P, _P, _P, _P]),
    'avae_tsne': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(AvaeTsneConfig)] + [_P] * 10),
    'avae_kmeans': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(AvaeKmeansConfig)] + [_P] * 8),
    'avae_gmm_fit': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(AvaeGmmConfig)] + [_P] * 17),
    'avae_gmm_score': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32] + [_P] * 6),
    'avae_silhouette': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(AvaeSilhouetteConfig), _P, C.POINTER(C.c_int32)] + [_P] * 7),
    'avae_dbscan': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(AvaeDbscanConfig), _P, _P, _P]),
    'avae_pca_fit': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(AvaePcaConfig), _P, _P, _P, _P]),
    'avae_pca_transform': (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P]),
    'avae_mmd': (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.POINTER(AvaeMmdConfig)] + [_P] * 9),
    'avae_mmd_relabel': (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_uint64]),
    # knobs used by tests / bench (not part of the reference-facing surface)
    'avae_set_option': (C.c_int, [_P, C.c_char_p, C.c_int]),
    'avae_debug_gemm': (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P] + [C.c_int] * 6 + [C.c_float, C.c_int, C.c_int]),
    'avae_debug_gemm_dyn': (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    'avae_debug_gemm_c16': (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    'avae_debug_gemm_tn16': (C.c_int, [_P, _P, _P, _P] + [C.c_int] * 6 + [C.c_float]),
    'avae_debug_softmax_ce': (C.c_int, [_P, _P, _P, C.c_int, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P, _P, _P, C.POINTER(C.c_int)]),
    'avae_debug_argmax_rows': (C.c_int, [_P, _P, _P, C.c_int, C.c_int]),
    'avae_debug_op': (C.c_int, [_P, C.c_char_p, C.POINTER(_P), C.POINTER(C.c_int64), C.POINTER(C.c_float)]),
    'avae_debug_op_layout': (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    'avae_debug_sample_rows': (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(AvaeSampleConfig), _P, _P]),
    'avae_debug_sample_rows_p': (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(AvaeSamplePConfig), _P, _P, _P, _P]),
    'avae_debug_beam_select': (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P]),
    'avae_timing_collect': (C.c_int, [_P, C.POINTER(C.c_double)]),
    'avae_debug_timing': (C.c_int, [_P, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]),
    'avae_debug_train_ce': (C.c_int, [_P, _P, C.c_int32, C.POINTER(C.c_int32)]),
    'avae_debug_stamps': (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    'avae_debug_present_ids': (C.c_int, [_P, C.POINTER(C.c_int32)]),
    'avae_debug_step_route': (C.c_int, [_P, C.POINTER(C.c_int32)]),
    'avae_debug_score_plan':(C.c_int, [_P, C.POINTER(C.c_int32)]),
    'avae_debug_row_expect': (C.c_int, [_P, C.POINTER(C.c_int32)]),
    'avae_debug_team_batch': (C.c_int, [C.c_int32]),
    'avae_debug_gemm_plan': (C.c_int, [_P, C.c_int32, _P]),
    'avae_debug_gemm_call': (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P] + [C.c_int] * 6 + [C.c_float, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P]),
    'avae_debug_gemm_forced': (C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P] + [C.c_int] * 6 + [C.c_float, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int,
                                         _P, _P, _P, _P]),
    'avae_debug_gemm_f32_form': (C.c_int, [C.c_int] * 14 + [C.POINTER(C.c_int32)]),
    'avae_debug_gemm16': (C.c_int, [_P] + [C.c_int] * 4 + [_P] * 6 + [C.c_int] * 6 + [C.c_float, C.c_int, _P, C.c_int, C.c_int]),
    'avae_debug_gemm_bf16_form': (C.c_int, [C.c_int] * 12 + [C.c_int64, C.POINTER(C.c_int32)]),
    'avae_debug_gru_plan': (C.c_int, [C.POINTER(C.c_int64), C.c_int, C.c_int, C.POINTER(C.c_int64)]),
    'avae_debug_decode_plan': (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'avae_debug_gru': (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int64)]),
    'avae_debug_sil_plan': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    'avae_debug_mmd_plan': (C.c_int, [C.c_int32] * 6 + [C.POINTER(C.c_int32), C.c_int32]),
    'avae_debug_dbscan_plan': (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    'avae_debug_pca_plan': (C.c_int, [C.c_int32] * 6 + [C.POINTER(C.c_int32)]),
    'avae_bucket_count': (C.c_int, [_P]),
    'avae_bucket_info': (C.c_int, [_P, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
}

_lib = None


def build(force=False, jobs=4):
    """compile the HIP sources for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.run(['make', '-C', CSRC, 'clean'], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(['make', '-C', CSRC, '-j%d' % jobs], check=True, stdout=subprocess.DEVNULL)
    return LIB_PATH


def load():
    """-> ctypes.CDLL with every entry point typed.  Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libargsim_vae.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the HIP path)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
