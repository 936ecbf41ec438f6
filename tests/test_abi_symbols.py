"""CPU test: the C-ABI library loads and exports every symbol include/ncf_abi.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _header():
    txt = open(os.path.join(ROOT, "include", "ncf_abi.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def _declared():
    return sorted(set(re.findall(r"\b(ncf_[a-z0-9_]+)\s*\(", _header())))


# the whole rule from a C type of the header to ctypes: a pointer is c_void_p (const char*: c_char_p), a scalar one of these
C_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
             "uint32_t": ctypes.c_uint32, "ncf_stream_t": ctypes.c_void_p}


def _ctype(decl, named, where):
    """The ctypes type of one C declarator: a return type (``named`` False) or a parameter, whose last word is its name."""
    words = decl.replace("*", " * ").split()
    if named and words[-1] != "*":
        words = words[:-1]
    if "*" in words:
        return ctypes.c_char_p if words == ["const", "char", "*"] else ctypes.c_void_p
    assert len(words) == 1 and words[0] in C_SCALARS, f"{where}: the C type {' '.join(words)!r} is outside the rule"
    return C_SCALARS[words[0]]


def _prototypes():
    """name -> (restype, argtypes) of every ``RET ncf_name(ARGS);`` of the header."""
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w \t*]*?)\b(ncf_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header()):
        assert name not in out, f"{name} is declared twice"
        params = [] if args.strip() in ("", "void") else [a.strip() for a in args.split(",")]
        out[name] = (_ctype(ret, False, name), [_ctype(p, True, f"{name}, argument {k}") for k, p in enumerate(params)])
    return out


def test_every_prototype_of_the_header_has_its_ctypes_signature():
    """Types, not only names: a float bound as c_int64, or an argument missing from the table, loads and runs and corrupts a launch."""
    from deeprecommendation_amd import native
    protos = _prototypes()
    assert set(protos) == set(_declared()), sorted(set(protos) ^ set(_declared()))          # nothing the parser could not read
    assert set(protos) == set(native.SIGNATURES)
    for name, (res, args) in protos.items():
        bound_res, bound_args = native.SIGNATURES[name]
        assert bound_res is res, f"{name}: returns {res.__name__}, bound as {bound_res.__name__}"
        assert len(bound_args) == len(args), f"{name}: {len(args)} arguments, {len(bound_args)} bound"
        for k, (want, have) in enumerate(zip(args, bound_args)):
            assert have is want, f"{name}, argument {k}: {want.__name__} in the header, bound as {have.__name__}"
        assert native.SIGNATURES[name] == (res, args)


def test_the_type_rule_refuses_a_type_it_does_not_list():
    assert _ctype("const float* dev_x", True, "t") is ctypes.c_void_p and _ctype("const char*", False, "t") is ctypes.c_char_p
    assert _ctype("int64_t n", True, "t") is ctypes.c_int64 and _ctype("size_t", False, "t") is ctypes.c_size_t
    for bad in ("double x", "unsigned n", "long n", "unsigned long long n"):
        with pytest.raises(AssertionError, match="outside the rule"):
            _ctype(bad, True, "t")


def _header_constants():
    txt = _header()
    found = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(NCF_[A-Z0-9_]+)[ \t]+(-?\d+)[ \t]*$", txt, flags=re.M)
    for body in re.findall(r"\benum\s+\w*\s*\{([^}]*)\}", txt):
        found += re.findall(r"\b(NCF_[A-Z0-9_]+)\s*=\s*(-?\d+)", body)
    out = {}
    for name, value in found:
        assert name not in out, f"{name} is defined twice"
        out[name] = int(value)
    return out


# header name -> what native.py holds for it: an attribute, or (a table of native.py, its key)
MIRRORED = {
    "NCF_F32": "NCF_F32", "NCF_BF16": "NCF_BF16",
    "NCF_OK": "NCF_OK", "NCF_EINVAL": "NCF_EINVAL", "NCF_EUNSUPPORTED": "NCF_EUNSUPPORTED", "NCF_ELAUNCH": "NCF_ELAUNCH",
    "NCF_EWORKSPACE": "NCF_EWORKSPACE",
    "NCF_ATT_MLP": "ATT_MLP", "NCF_ATT_LINEAR": "ATT_LINEAR", "NCF_ATT_COS": "ATT_COS", "NCF_ATT_MLP_SCALED": "ATT_MLP_SCALED",
    "NCF_ATT_SCALE_LOG2": "ATT_SCALE_LOG2",
    "NCF_ALS_MAX_FACTORS": "ALS_MAX_FACTORS", "NCF_ALS_GRAM_ROWS": "ALS_GRAM_ROWS", "NCF_ALS_SEG": "ALS_SEG",
    "NCF_EASE_BLOCK": "EASE_BLOCK",
    "NCF_UNSEEN_MAX_K": "UNSEEN_MAX_K", "NCF_UNSEEN_LANE_K": "UNSEEN_LANE_K",
    "NCF_KMF_FLAG_ID": "KMF_FLAG_ID", "NCF_KMF_FLAG_BLOCK": "KMF_FLAG_BLOCK", "NCF_KMF_FLAG_PTR": "KMF_FLAG_PTR",
    "NCF_ALS_FLAG_COL": "ALS_FLAG_COL", "NCF_ALS_FLAG_PTR": "ALS_FLAG_PTR", "NCF_ALS_FLAG_ORDER": "ALS_FLAG_ORDER",
    "NCF_ALS_FLAG_VAL": "ALS_FLAG_VAL", "NCF_ALS_FLAG_PIVOT": "ALS_FLAG_PIVOT",
    "NCF_EASE_FLAG_ORDER": "EASE_FLAG_ORDER", "NCF_EASE_FLAG_PIVOT": "EASE_FLAG_PIVOT",
    "NCF_UNSEEN_FLAG_PICK": "UNSEEN_FLAG_PICK", "NCF_UNSEEN_FLAG_FEW": "UNSEEN_FLAG_FEW",
    "NCF_RANKING_TOPK_ROWS": ("RANKING_ENTRIES", "topk_rows"), "NCF_RANKING_RANK_ROWS": ("RANKING_ENTRIES", "rank_rows"),
    "NCF_RANKING_DOT_TOPK": ("RANKING_ENTRIES", "dot_topk"), "NCF_RANKING_DOT_RANK": ("RANKING_ENTRIES", "dot_rank"),
    "NCF_RANKING_MLP_TOPK": ("RANKING_ENTRIES", "mlp_topk"), "NCF_RANKING_MLP_RANK": ("RANKING_ENTRIES", "mlp_rank"),
    "NCF_DOT_SOFTMAX_LSE": ("DOT_SOFTMAX_KINDS", "lse"), "NCF_DOT_SOFTMAX_GRAD_ROWS": ("DOT_SOFTMAX_KINDS", "grad_rows"),
    "NCF_DOT_SOFTMAX_GRAD_ITEMS": ("DOT_SOFTMAX_KINDS", "grad_items"),
}


def test_every_constant_native_mirrors_has_the_value_of_the_header():
    from deeprecommendation_amd import native
    header = _header_constants()
    for name, mirror in MIRRORED.items():
        assert name in header, f"{name} is not an integer #define or enum entry of the header"
        value = getattr(native, mirror) if isinstance(mirror, str) else getattr(native, mirror[0])[mirror[1]]
        assert value == header[name], f"{name} = {header[name]} in the header, native holds {value}"
    # every flag bit, ranking entry and softmax kind of the header is paired above, and the two name maps hold nothing else
    for name in header:
        if "_FLAG_" in name or name.startswith(("NCF_RANKING_", "NCF_DOT_SOFTMAX_")):
            assert name in MIRRORED, f"{name} of the header has no mirror listed here"
    for table in ("RANKING_ENTRIES", "DOT_SOFTMAX_KINDS"):
        assert sorted(getattr(native, table)) == sorted(m[1] for m in MIRRORED.values() if not isinstance(m, str) and m[0] == table)
    # and the rows of a word with several meanings are the header's bits of that word, each once
    for kind, prefix in (("kmf", "NCF_KMF_FLAG_"), ("als", "NCF_ALS_FLAG_"), ("ease", "NCF_EASE_FLAG_"), ("unseen", "NCF_UNSEEN_FLAG_")):
        rows = native._FLAG_WORDS[kind][1]
        assert sorted(bit for bit, _, _ in rows) == sorted(v for name, v in header.items() if name.startswith(prefix)), kind


def test_header_symbols_exported_and_bound():
    from deeprecommendation_amd import native
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = native.load_library()
    declared = _declared()
    assert len(declared) >= 15
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in ncf_abi.h but not exported"
        assert name in native.SIGNATURES, f"{name} has no ctypes signature"
    assert set(native.SIGNATURES) == set(declared)
    assert lib.ncf_version() == 1
    assert lib.ncf_build_arch() == b"gfx950"


def test_missing_library_fails_loudly(tmp_path):
    from deeprecommendation_amd import native
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.load_library(str(tmp_path / "nope.so"))


def test_cpu_tensors_are_rejected_in_eval():
    import torch
    from deeprecommendation_amd.neural_collaborative_filtering.models.basic_ncf import BasicNCF
    m = BasicNCF(item_dim=10, user_dim=12, item_emb=8, user_emb=8, mlp_dense_layers=[16]).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(3, dtype=torch.long), torch.zeros(3, dtype=torch.long))


def test_option_table_matches_the_binding():
    """ncf_set_option / ncf_get_option are host-only: every symbolic value the Python binding knows is accepted by the library's option
    table and reads back; a value outside an option's range and an unknown option are refused with the error string set."""
    from deeprecommendation_amd import native
    lib = native.load_library()
    try:
        for name, values in native.OPTION_VALUES.items():
            for sym, val in values.items():
                native.set_option(name, sym)
                assert native.get_option(name) == val, (name, sym)
            top = max(values.values())
            assert lib.ncf_set_option(name.encode(), top + 50) != native.NCF_OK
            assert name.encode() in lib.ncf_last_error()
        assert lib.ncf_set_option(b"no_such_option", 1) != native.NCF_OK
        with pytest.raises(ValueError):
            native.set_option("bf16_kernel", "no_such_kernel")
    finally:
        for name in native.OPTION_VALUES:
            native.set_option(name, "auto")


def test_library_carries_the_id_of_its_sources_and_a_stale_one_is_refused(tmp_path, monkeypatch):
    """ncf_build_id(): the library embeds a hash of every source / header / flag it was built from; needs_build() compares ids (not
    mtimes), and the binding refuses a library whose id is not that of the sources next to it."""
    from deeprecommendation_amd import native
    from deeprecommendation_amd.csrc import build as b
    lib = native.load_library()
    assert lib.ncf_build_id().decode() == b.source_id() == b.library_id()
    assert not b.needs_build()
    monkeypatch.setattr(b, "source_id", lambda: "0123456789abcdef")       # as if a source had been edited
    assert b.needs_build()
    with pytest.raises(RuntimeError, match="stale"):
        native._check_build_id(lib, "libncf_hip.so")


def test_every_attribute_of_native_the_repository_names_still_resolves():
    """The outcome of the sweep that followed the fold of native.py's flag tables, workspaces, plan queries and attention operands:
    the three retired flag tables are gone, and every ``native.<name>`` that a Python file of the repository writes — the package, the
    tests, the tools, the benchmarks — is an attribute of the module."""
    from deeprecommendation_amd import native
    for retired in ("_FLAG_BITS", "_EASE_FLAG_BITS", "_UNSEEN_FLAG_BITS"):
        assert not hasattr(native, retired), retired
    named = {}
    for top in ("deeprecommendation_amd", "tests", "tools", "oracle", "."):
        for folder, _, files in os.walk(os.path.join(ROOT, top)) if top != "." else [(ROOT, [], os.listdir(ROOT))]:
            for f in files:
                if f.endswith(".py"):
                    path = os.path.join(folder, f)
                    for name in re.findall(r"\bnative\.([A-Za-z_]\w*)(?![\w*])", open(path, errors="replace").read()):
                        named.setdefault(name, os.path.relpath(path, ROOT))
    named.pop("py", None)                                                  # "native.py", the file
    assert len(named) > 150
    missing = {name: path for name, path in named.items() if not hasattr(native, name)}
    assert not missing, missing
