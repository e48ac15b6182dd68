# -*- coding: utf-8 -*-
"""ctypes binding of the C-ABI (include/celerite2_amd.h, celerite2_amd_linear.h, celerite2_amd_periodogram.h,
celerite2_amd_transit.h, celerite2_amd_kepler.h, celerite2_amd_trials.h, celerite2_amd_shapes.h,
celerite2_amd_harmonics.h, celerite2_amd_harmonic_trials.h, celerite2_amd_filter.h, celerite2_amd_filter_rev.h,
celerite2_amd_filter_stream_rev.h and celerite2_amd_filter_draw.h).

There is NO CPU fallback: if libcelerite2_amd.so is missing or no HIP device is
visible, the product path raises -- it never routes through oracle/.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# override: A/B builds.  Whatever library is chosen, it is bound with THIS tree's header (the ABI of an A/B pair is one).
LIB_PATH = os.environ.get("C2_LIB_PATH", os.path.join(_HERE, "libcelerite2_amd.so"))
HEADER = os.path.join(os.path.dirname(_HERE), "include", "celerite2_amd.h")   # = build.INCLUDE: the build is in-tree
LINEAR_HEADER = os.path.join(os.path.dirname(_HERE), "include", "celerite2_amd_linear.h")   # linear mean models
PERIODOGRAM_HEADER = os.path.join(os.path.dirname(_HERE), "include", "celerite2_amd_periodogram.h")   # the periodogram
TRANSIT_HEADER = os.path.join(os.path.dirname(_HERE), "include", "celerite2_amd_transit.h")   # the transit search
KEPLER_HEADER = os.path.join(os.path.dirname(_HERE), "include", "celerite2_amd_kepler.h")   # the Keplerian search
TRIALS_HEADER = os.path.join(os.path.dirname(_HERE), "include", "celerite2_amd_trials.h")   # projections on trial columns
SHAPES_HEADER = os.path.join(os.path.dirname(_HERE), "include", "celerite2_amd_shapes.h")   # the tabulated-shape search
HARMONICS_HEADER = os.path.join(os.path.dirname(_HERE), "include", "celerite2_amd_harmonics.h")   # the multi-harmonic periodogram
HARMONIC_TRIALS_HEADER = os.path.join(os.path.dirname(_HERE), "include", "celerite2_amd_harmonic_trials.h")   # ... and its null draws
FILTER_HEADER = os.path.join(os.path.dirname(_HERE), "include", "celerite2_amd_filter.h")   # streaming updates
FILTER_REV_HEADER = os.path.join(os.path.dirname(_HERE), "include", "celerite2_amd_filter_rev.h")   # ... and their reverse
FILTER_STREAM_REV_HEADER = os.path.join(os.path.dirname(_HERE), "include", "celerite2_amd_filter_stream_rev.h")   # ... of absorb and forecast
FILTER_DRAW_HEADER = os.path.join(os.path.dirname(_HERE), "include", "celerite2_amd_filter_draw.h")   # forecast sample paths


class BackendError(RuntimeError):
    pass


class Pointer(ctypes.c_void_p):
    """Every pointer parameter of the header except `const char *`: a tensor (anything with .data_ptr()), None, an int,
    a c_void_p, byref(...) or ndarray.ctypes.data_as(c_void_p) -- but no str / bytes, which c_void_p would take."""

    @classmethod
    def from_param(cls, x, _void_p=ctypes.c_void_p):
        if x is None or type(x) is _void_p:
            return x
        try:
            return _void_p(x.data_ptr())
        except AttributeError:
            if isinstance(x, (str, bytes)):
                raise TypeError("a pointer argument, not %s" % type(x).__name__)
            return _void_p.from_param(x)


# The C types of the header's prototypes (parameters and return values).  A prototype that uses another one fails at load.
_CTYPES = {"void": None, "int": ctypes.c_int, "double": ctypes.c_double, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p}
_CTYPES.update(dict.fromkeys(("double *", "const double *", "int32_t *", "const int32_t *", "int *", "int64_t *", "void *",
                              "c2_stream_t", "const char **", "const c2_term_program *", "const c2_term_expr *"), Pointer))


def _header(path=None):
    """A public header (default: include/celerite2_amd.h) without its comments."""
    path = HEADER if path is None else path
    if not os.path.exists(path):
        raise BackendError("celerite2_amd: %s not found -- the Python binding takes its prototypes from it" % path)
    return re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)


def _ctype(text, name):
    text = " ".join(text.replace("*", " * ").split()).replace("* *", "**")
    if text not in _CTYPES:
        raise BackendError("celerite2_amd: %s: no ctypes type for %r (celerite2_amd/_lib.py, _CTYPES)" % (name, text))
    return _CTYPES[text]


def _prototypes(header):
    """name -> (restype, argtypes) of every `ret c2[h]_name(params);` the header declares."""
    protos = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?\w+[\s*]+)(c2h?_\w+)\s*\(([^()]*)\)\s*;", header, flags=re.M):
        params = [] if params.strip() == "void" else [re.sub(r"\w+$", "", p.strip()) for p in params.split(",")]
        protos[name] = (_ctype(ret, name), [_ctype(p, name) for p in params])
    return protos


globals().update({k: int(v) for k, v in re.findall(r"^#define\s+(C2_(?:OK|ERR_\w+|MAX_WIDTH|FAST_WIDTH))\s+\(?(-?\d+)\)?\s*$",
                                                     _header(), flags=re.M)})

# Every symbol include/celerite2_amd.h declares (checked by tests/test_abi.py).
SYMBOLS = [
    "c2_version", "c2_device_count", "c2_last_error",
    "c2_factor", "c2_solve_lower", "c2_solve_upper", "c2_matmul_lower", "c2_matmul_upper",
    "c2_general_matmul_lower", "c2_general_matmul_upper", "c2_factor_rev",
    "c2_solve_lower_rev", "c2_solve_upper_rev", "c2_matmul_lower_rev", "c2_matmul_upper_rev",
    "c2_get_celerite_matrices", "c2_kernel_values", "c2_colsumsq_over_d", "c2_loglik", "c2_loglik_grad_workspace_bytes", "c2_loglik_grad", "c2_condition", "c2_dot_tril",
    "c2_kron_loglik_workspace_bytes", "c2_kron_loglik", "c2_kron_loglik_grad",
    "c2_loglik_terms_workspace_bytes", "c2_loglik_terms", "c2_loglik_terms_grad",
    "c2_term_coefficients", "c2_term_coefficients_rev", "c2_noise_mean_apply", "c2_noise_mean_rev",
    "c2_term_expr_workspace_bytes", "c2_term_expr_coefficients", "c2_term_expr_coefficients_rev",
    "c2_noise_mean_shift_apply", "c2_noise_mean_shift_rev", "c2_inverse_diag", "c2_explained_variance",
    "c2_prior_draw", "c2_inverse_diag_fwd", "c2_inverse_diag_rev",
    "c2_get_celerite_matrices_rev_workspace_bytes", "c2_get_celerite_matrices_rev",
    "c2_general_matmul_lower_rev", "c2_general_matmul_upper_rev",
    "c2_explained_variance_fwd", "c2_explained_variance_rev",
    "c2h_factor", "c2h_solve_lower", "c2h_solve_upper", "c2h_matmul_lower", "c2h_matmul_upper",
    "c2h_general_matmul_lower", "c2h_general_matmul_upper", "c2h_factor_rev",
    "c2h_solve_lower_rev", "c2h_solve_upper_rev", "c2h_matmul_lower_rev", "c2h_matmul_upper_rev",
    "c2h_get_celerite_matrices", "c2h_release_thread_cache",
    "c2_set_option", "c2_get_option", "c2_option_count", "c2_option_info", "c2_options_reload_env",
]

# Every symbol include/celerite2_amd_linear.h declares (checked by tests/test_linear_model.py).
LINEAR_SYMBOLS = ["c2_whitened_gram"]

# Every symbol include/celerite2_amd_periodogram.h declares (checked by tests/test_periodogram.py).
PERIODOGRAM_SYMBOLS = ["c2_whitened_sinusoids"]

# Every symbol include/celerite2_amd_transit.h declares (checked by tests/test_transit.py).
TRANSIT_SYMBOLS = ["c2_whitened_transits"]

# Every symbol include/celerite2_amd_kepler.h declares (checked by tests/test_kepler.py).
KEPLER_SYMBOLS = ["c2_whitened_keplerians"]

# Every symbol include/celerite2_amd_trials.h declares (checked by tests/test_significance.py).
TRIALS_SYMBOLS = ["c2_trial_projections"]

# Every symbol include/celerite2_amd_shapes.h declares (checked by tests/test_shapes.py).
SHAPES_SYMBOLS = ["c2_whitened_shapes", "c2_shape_projections"]

# Every symbol include/celerite2_amd_harmonics.h declares (checked by tests/test_harmonics.py).
HARMONICS_SYMBOLS = ["c2_whitened_harmonics"]

# Every symbol include/celerite2_amd_harmonic_trials.h declares (checked by tests/test_harmonic_significance.py).
HARMONIC_TRIALS_SYMBOLS = ["c2_harmonic_projections", "c2_harmonic_null_chi2"]

# Every symbol include/celerite2_amd_filter.h declares (checked by tests/test_filter.py).
FILTER_SYMBOLS = ["c2_filter_state_words", "c2_filter_append", "c2_filter_absorb", "c2_filter_forecast"]

# Every symbol include/celerite2_amd_filter_rev.h declares (checked by tests/test_filter_rev.py).
FILTER_REV_SYMBOLS = ["c2_filter_rev_workspace_words", "c2_filter_append_rev"]

# Every symbol include/celerite2_amd_filter_stream_rev.h declares (checked by tests/test_filter_stream_rev.py).  (Not a
# *SYMBOLS list: those are the census of tests/large_batch_cases.py; tests/test_gpu_filter_stream_rev.py runs these two at
# 70000 series itself.)
FILTER_STREAM_REV_EXPORTS = ["c2_filter_forecast_rev", "c2_filter_absorb_rev"]

# Every symbol include/celerite2_amd_filter_draw.h declares (checked by tests/test_filter_draw.py).  (Not a *SYMBOLS list
# either: tests/test_gpu_filter_draw.py runs the draw at 70000 series itself.)
FILTER_DRAW_EXPORTS = ["c2_filter_draw_chunk", "c2_filter_draw"]

_lib = None
_env_names = ()      # environment variables of the option table (c2_option_info)
_env_seen = None     # their values when the table was last (re)loaded


def _sync_env(lib):
    """The C library reads its dispatch options from the environment ONCE, when it is loaded, and never calls getenv
    afterwards (c2_dispatch.hpp).  This ctypes layer additionally follows the process environment when it SEES one of the
    table's variables change between two calls -- what the test-suite and the A/B tools rely on when they edit os.environ
    at run time -- and applies exactly the variables that changed (c2_set_option each), so values an application set
    through set_option() for OTHER options survive an unrelated monkeypatch.setenv.  Applications use set_option()."""
    global _env_seen
    now = tuple(os.environ.get(n) for n in _env_names)
    if now != _env_seen:
        for name, old, new in zip(_env_names, _env_seen or (None,) * len(_env_names), now):
            if old != new:
                # unset or unparsable -> back to the table's default, as at load time
                if lib.c2_set_option(name.encode(), None if not new else new.encode()) != C2_OK:
                    lib.c2_set_option(name.encode(), None)
        _env_seen = now


def set_option(name, value=None):
    """c2_set_option: `name` = option name or its environment variable; value None = back to the default / automatic."""
    lib = load()
    rc = lib.c2_set_option(str(name).encode(), None if value is None else str(value).encode())
    if rc != C2_OK:
        raise ValueError("celerite2_amd: unknown option %r or unparsable value %r" % (name, value))


def options():
    """The dispatch table: a list of dicts (name, env, default, switch, value, is_set, doc, measured)."""
    lib = load()
    out = []
    for i in range(lib.c2_option_count()):
        name, env, doc, src = (ctypes.c_char_p() for _ in range(4))
        dflt, sw = ctypes.c_double(), ctypes.c_int()
        lib.c2_option_info(i, ctypes.byref(name), ctypes.byref(env), ctypes.byref(dflt), ctypes.byref(sw), ctypes.byref(doc),
                           ctypes.byref(src))
        val, st = ctypes.c_double(), ctypes.c_int()
        lib.c2_get_option(name.value, ctypes.byref(val), ctypes.byref(st))
        out.append(dict(name=name.value.decode(), env=env.value.decode(), default=dflt.value, switch=bool(sw.value),
                        value=val.value, is_set=bool(st.value), doc=doc.value.decode(), measured=src.value.decode()))
    return out


def load():
    """Load libcelerite2_amd.so (after torch, so both share one HIP runtime)."""
    global _lib, _env_names, _env_seen
    if _lib is not None:
        _sync_env(_lib)
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BackendError(
            "celerite2_amd: %s not found -- build it with `python -m celerite2_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH
        )
    try:  # torch bundles libamdhip64.so.7; importing it first makes the soname resolve to that copy
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is plumbing, not required for the C-ABI itself
        pass
    lib = ctypes.CDLL(LIB_PATH)
    protos = _prototypes(_header())
    protos.update(_prototypes(_header(LINEAR_HEADER)))
    protos.update(_prototypes(_header(PERIODOGRAM_HEADER)))
    protos.update(_prototypes(_header(TRANSIT_HEADER)))
    protos.update(_prototypes(_header(KEPLER_HEADER)))
    protos.update(_prototypes(_header(TRIALS_HEADER)))
    protos.update(_prototypes(_header(SHAPES_HEADER)))
    protos.update(_prototypes(_header(HARMONICS_HEADER)))
    protos.update(_prototypes(_header(HARMONIC_TRIALS_HEADER)))
    protos.update(_prototypes(_header(FILTER_HEADER)))
    protos.update(_prototypes(_header(FILTER_REV_HEADER)))
    protos.update(_prototypes(_header(FILTER_STREAM_REV_HEADER)))
    protos.update(_prototypes(_header(FILTER_DRAW_HEADER)))
    for name, (restype, argtypes) in protos.items():
        # (built with parameter flags, "input" each: a call then takes EXACTLY that many arguments -- argtypes alone let a
        # cdecl function take more)
        setattr(lib, name, ctypes.CFUNCTYPE(restype, *argtypes)((name, lib), ((1,),) * len(argtypes)))
    _lib = lib
    names = []
    for i in range(lib.c2_option_count()):
        env = ctypes.c_char_p()
        lib.c2_option_info(i, None, ctypes.byref(env), None, None, None, None)
        names.append(env.value.decode())
    _env_names = tuple(names)
    _env_seen = tuple(os.environ.get(n) for n in _env_names)
    return lib


def check(rc, what):
    if rc == C2_OK:
        return
    lib = load()
    if rc == C2_ERR_INVALID:
        raise ValueError("celerite2_amd.%s: invalid shape / null argument" % what)
    if rc == C2_ERR_UNSUPPORTED:
        raise ValueError("celerite2_amd.%s: width not supported (J <= %d; the 2-D and coefficient-level extensions: J <= 32)"
                         % (what, C2_MAX_WIDTH))
    raise BackendError("celerite2_amd.%s: HIP error: %s" % (what, lib.c2_last_error().decode()))
