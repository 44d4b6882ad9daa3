"""CPU test of the Prodigy boundary (the pattern of tests/test_abi_step_cache.py): include/fk.h declares the four kernels, the
workspace size and the state slots, the library exports them, libfk.py has their prototypes and slot names, and ops wraps them."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fk_prodigy_begin", "fk_prodigy_moments", "fk_prodigy_update_d", "fk_prodigy_apply", "fk_prodigy_ws_doubles")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fk.h")).read(), flags=re.S)


def test_prodigy_symbols_are_declared_exported_and_bound():
    from gpt_image_edit_amd import libfk
    if not os.path.exists(libfk.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    declared = set(re.findall(r"\b(fk_[a-z0-9_]+)\s*\(", _header()))
    lib = libfk.load()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/fk.h"
        assert hasattr(lib, name), f"{name} is not exported by libfk"
        assert name in libfk.SIGNATURES, f"{name} has no ctypes signature"
    assert lib.fk_prodigy_ws_doubles() == 2 * 2048


def test_signatures_are_the_declared_ones():
    """Argument by argument: the C declaration's parameter types against the ctypes prototype."""
    from gpt_image_edit_amd import libfk
    kinds = {"const void*": libfk.c_vp, "void*": libfk.c_vp, "float*": libfk.c_vp, "const float*": libfk.c_vp, "double*": libfk.c_vp,
             "const double*": libfk.c_vp, "fk_stream_t": libfk.c_vp, "int64_t": libfk.c_i64, "int32_t": libfk.c_i32,
             "float": libfk.c_f32, "double": libfk.c_f64}
    src = _header()
    for name in NEW[:4]:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            typ = re.sub(r"\s*\b\w+$", "", " ".join(arg.split()))          # drop the parameter's name
            want.append(kinds[typ])
        res, args = libfk.SIGNATURES[name]
        assert res is libfk.c_i32 and args == want, (name, args, want)
    assert libfk.SIGNATURES["fk_prodigy_ws_doubles"] == (libfk.c_i64, [])
    assert [len(libfk.SIGNATURES[n][1]) for n in NEW[:4]] == [7, 21, 5, 10]


def test_state_slots_match_the_header():
    from gpt_image_edit_amd import libfk
    slots = dict((n.lower(), int(v)) for n, v in re.findall(r"\bFK_PRODIGY_([A-Z_0-9]+)\s*=\s*(\d+)", _header()))
    assert slots.pop("state_doubles") == len(libfk.FK_PRODIGY_SLOTS) == 10
    assert [k for k, _ in sorted(slots.items(), key=lambda kv: kv[1])] == list(libfk.FK_PRODIGY_SLOTS)
    assert libfk.FK_PRODIGY_SLOTS == ("d", "d_max", "d_numerator", "d_denom", "d_hat", "dlr", "k", "skipped", "sum_dot", "sum_abs")
    from gpt_image_edit_amd import zero
    assert zero.PRODIGY_SLOTS == libfk.FK_PRODIGY_SLOTS


def test_ops_wrappers():
    from gpt_image_edit_amd import ops
    sig = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert sig(ops.prodigy_begin) == ["state", "lr", "betas", "beta3", "use_bias_correction"]
    assert sig(ops.prodigy_moments)[:7] == ["master", "p0", "grad", "m", "v", "s", "state"]
    assert {"grad_sumsq", "max_grad_norm", "grad_scale", "decouple", "safeguard_warmup", "d0", "ws"} <= set(sig(ops.prodigy_moments))
    assert sig(ops.prodigy_update_d) == ["state", "d0", "d_coef", "growth_rate"]
    assert sig(ops.prodigy_apply) == ["master", "m", "v", "state", "eps", "weight_decay", "decouple", "param_bf16"]
    assert sig(ops.prodigy_state) == ["buf"]
    assert inspect.signature(ops.prodigy_update_d).parameters["growth_rate"].default == float("inf")


def test_new_file_is_built_by_the_makefile():
    mk = open(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "gpt_image_edit_amd", "csrc", "prodigy.hip"))
    assert "$(wildcard *.hip)" in mk or "prodigy.hip" in mk
