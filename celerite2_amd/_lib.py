# -*- coding: utf-8 -*-
"""ctypes binding of the C-ABI: every public header under include/ has one record in HEADERS below, and the binding, the
build's staleness list, the ABI tests (tests/test_abi.py) and the census of entry points (tests/test_large_batch_table.py)
all read that table.  A new public header is one more record.

There is NO CPU fallback: if libcelerite2_amd.so is missing or no HIP device is
visible, the product path raises -- it never routes through oracle/.
"""
import collections
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# override: A/B builds.  Whatever library is chosen, it is bound with THIS tree's headers (the ABI of an A/B pair is one).
LIB_PATH = os.environ.get("C2_LIB_PATH", os.path.join(_HERE, "libcelerite2_amd.so"))

# One public header: its file under include/, the C symbols it declares in the header's order (hand-written: the pin the
# header is compared against) and the public names of ops.py that belong to it (None: ops.__all__).
Header = collections.namedtuple("Header", "file symbols ops")

HEADERS = {
    "main": Header("celerite2_amd.h", [
        "c2_version", "c2_device_count", "c2_last_error",
        "c2_set_option", "c2_get_option", "c2_option_count", "c2_option_info", "c2_options_reload_env",
        "c2_factor", "c2_solve_lower", "c2_solve_upper", "c2_matmul_lower", "c2_matmul_upper",
        "c2_general_matmul_lower", "c2_general_matmul_upper", "c2_factor_rev",
        "c2_solve_lower_rev", "c2_solve_upper_rev", "c2_matmul_lower_rev", "c2_matmul_upper_rev",
        "c2_get_celerite_matrices", "c2_kernel_values", "c2_colsumsq_over_d", "c2_loglik", "c2_loglik_grad_workspace_bytes",
        "c2_loglik_grad", "c2_condition",
        "c2_kron_loglik_workspace_bytes", "c2_kron_loglik", "c2_kron_loglik_grad",
        "c2_loglik_terms_workspace_bytes", "c2_loglik_terms", "c2_loglik_terms_grad",
        "c2_term_coefficients", "c2_term_coefficients_rev", "c2_noise_mean_apply", "c2_noise_mean_rev",
        "c2_term_expr_workspace_bytes", "c2_term_expr_coefficients", "c2_term_expr_coefficients_rev",
        "c2_noise_mean_shift_apply", "c2_noise_mean_shift_rev", "c2_dot_tril",
        "c2_inverse_diag", "c2_inverse_diag_fwd", "c2_inverse_diag_rev",
        "c2_get_celerite_matrices_rev_workspace_bytes", "c2_get_celerite_matrices_rev",
        "c2_explained_variance", "c2_explained_variance_fwd", "c2_explained_variance_rev", "c2_prior_draw",
        "c2_general_matmul_lower_rev", "c2_general_matmul_upper_rev",
        "c2h_factor", "c2h_solve_lower", "c2h_solve_upper", "c2h_matmul_lower", "c2h_matmul_upper",
        "c2h_general_matmul_lower", "c2h_general_matmul_upper", "c2h_factor_rev",
        "c2h_solve_lower_rev", "c2h_solve_upper_rev", "c2h_matmul_lower_rev", "c2h_matmul_upper_rev",
        "c2h_get_celerite_matrices", "c2h_release_thread_cache",
    ], None),
    "linear": Header("celerite2_amd_linear.h", ["c2_whitened_gram"], ["whitened_gram"]),   # linear mean models
    "periodogram": Header("celerite2_amd_periodogram.h", ["c2_whitened_sinusoids"], ["whitened_sinusoids"]),
    "transit": Header("celerite2_amd_transit.h", ["c2_whitened_transits"], ["whitened_transits"]),   # the transit search
    "kepler": Header("celerite2_amd_kepler.h", ["c2_whitened_keplerians"], ["whitened_keplerians"]),   # the Keplerian search
    "trials": Header("celerite2_amd_trials.h", ["c2_trial_projections"], ["trial_projections"]),   # projections on trial columns
    "shapes": Header("celerite2_amd_shapes.h", ["c2_whitened_shapes", "c2_shape_projections"],   # the tabulated-shape search
                     ["whitened_shapes", "shape_projections"]),
    "harmonics": Header("celerite2_amd_harmonics.h", ["c2_whitened_harmonics"], ["whitened_harmonics"]),   # the multi-harmonic periodogram
    "harmonic_trials": Header("celerite2_amd_harmonic_trials.h", ["c2_harmonic_projections", "c2_harmonic_null_chi2"],   # ... and its null draws
                              ["harmonic_projections", "harmonic_null_chi2"]),
    "filter": Header("celerite2_amd_filter.h",   # streaming updates
                     ["c2_filter_state_words", "c2_filter_append", "c2_filter_absorb", "c2_filter_forecast"],
                     ["filter_state_words", "filter_init", "filter_append", "filter_absorb", "filter_forecast"]),
    "filter_rev": Header("celerite2_amd_filter_rev.h", ["c2_filter_rev_workspace_words", "c2_filter_append_rev"],   # ... and their reverse
                         ["filter_rev_workspace_words", "filter_append_rev"]),
    "filter_stream_rev": Header("celerite2_amd_filter_stream_rev.h", ["c2_filter_forecast_rev", "c2_filter_absorb_rev"],   # ... of absorb and forecast
                                ["filter_forecast_rev", "filter_absorb_rev"]),
    "filter_draw": Header("celerite2_amd_filter_draw.h", ["c2_filter_draw_chunk", "c2_filter_draw"],   # forecast sample paths
                          ["filter_draw_chunk", "filter_draw"]),
}


def header_path(key):
    return os.path.join(os.path.dirname(_HERE), "include", HEADERS[key].file)   # (the build is in-tree)


class BackendError(RuntimeError):
    pass


def header_text(key):
    """A public header without its comments."""
    path = header_path(key)
    if not os.path.exists(path):
        raise BackendError("celerite2_amd: %s not found -- the Python binding takes its prototypes from it" % path)
    return re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)


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
_CTYPES.update(dict.fromkeys(("double *", "const double *", "int32_t *", "const int32_t *", "int *", "int64_t *", "const int64_t *", "void *",
                              "c2_stream_t", "const char **", "const c2_term_program *", "const c2_term_expr *"), Pointer))


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
                                                     header_text("main"), flags=re.M)})

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
    protos = {}
    for key in HEADERS:
        protos.update(_prototypes(header_text(key)))
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
