"""The ledger behind include/mhx.h's promise that tests/test_guard_pages.py and the *_guard_cases.py scripts hold every `_dev`
entry point to its argument list: every such symbol the header declares is called in some tests/*guard_cases.py, or stands in
the one table of exemptions below with its reason.  Runs without a GPU: it reads the header, mhx_api.hip and the scripts.

A symbol counts as called when a guard script holds `lib.<symbol>(` or `ctx.<symbol without "mhx_" and a trailing "_typed">(`,
the two ways those scripts reach the C ABI (the binding's methods of that name are thin calls of the symbol).
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mhx.h")
API = os.path.join(ROOT, "datasketch_amd", "csrc", "mhx_api.hip")

NEEDS_RANKS = "needs several ranks; covered by the rank tests (tests/rank_c3.py, tests/rank_c5.py)"
# symbol -> (the symbol whose guard cases stand for it, or None, and why).  A forwarding wrapper is one whose whole body in
# mhx_api.hip is `return <target>(...);` -- the test checks that it still is, and that the target is covered.
EXEMPT = {
    "mhx_comm_allgather_dev": (None, NEEDS_RANKS),
    "mhx_comm_allgatherv_dev": (None, NEEDS_RANKS),
    "mhx_comm_exchange_dev": (None, NEEDS_RANKS),
    "mhx_band_digests_dev": ("mhx_band_digests_layout_dev", "forwards with MHX_U64 and MHX_ROW_MAJOR"),
    "mhx_band_digests_dev_typed": ("mhx_band_digests_layout_dev", "forwards with MHX_ROW_MAJOR"),
    "mhx_bbit_pack_dev": ("mhx_bbit_pack_dev_typed", "forwards with MHX_U64"),
    "mhx_jaccard_pairs_dev": ("mhx_jaccard_pairs_dev_typed", "forwards with MHX_U64"),
    "mhx_lean_serialize_dev": ("mhx_lean_serialize_dev_typed", "forwards with MHX_U64 and MHX_LITTLE_ENDIAN"),
    "mhx_lsh_sort_bands_dev": ("mhx_lsh_sort_bands_dev_typed", "forwards with MHX_U64"),
    "mhx_lsh_sort_digests_dev": ("mhx_lsh_sort_digests_layout_dev", "forwards with MHX_ROW_MAJOR"),
}

_DECLARED = re.compile(r"^MHX_API\w*\s+int\s+(mhx_\w+_dev(?:_typed)?)\b\s*\(", re.M)


def declared_symbols(header_text):
    return sorted(set(_DECLARED.findall(header_text)))


def guard_scripts():
    return sorted(glob.glob(os.path.join(ROOT, "tests", "*guard_cases.py")))


def called_in(text, symbol):
    short = re.sub(r"_typed$", "", symbol[len("mhx_"):])
    return re.search(r"\blib\." + symbol + r"\(", text) is not None or re.search(r"\bctx\." + short + r"\(", text) is not None


def forwards_to(api_text, symbol):
    """The callee when the whole body of `symbol` in mhx_api.hip is one `return callee(...);`, else None."""
    m = re.search(r"^int " + symbol + r"\([^{;]*\)\s*\{\s*return\s+(mhx_\w+)\([^;{}]*\);\s*\}", api_text, re.M)
    return m.group(1) if m else None


def missing_symbols(header_text, scripts_text):
    """Declared `_dev` symbols that no guard script calls and no exemption stands for."""
    missing = set()
    for symbol in declared_symbols(header_text):
        if symbol in EXEMPT:
            target = EXEMPT[symbol][0]
            if target is not None and not called_in(scripts_text, target):
                missing.add(target)
        elif not called_in(scripts_text, symbol):
            missing.add(symbol)
    return sorted(missing)


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def test_the_pattern_takes_device_entry_points_only():
    text = ("MHX_API int mhx_ctx_device_info(mhx_ctx *ctx);\nMHX_API int mhx_dev_alloc(mhx_ctx *ctx);\n"
            "MHX_API_TOPK int mhx_jaccard_topk_dev(mhx_ctx *ctx,\n/* see mhx_hidden_dev( */\nMHX_API int mhx_bbit_pack_dev_typed(mhx_ctx *ctx);\n"
            "MHX_API int mhx_bbit_pack(mhx_ctx *ctx);\n")
    assert declared_symbols(text) == ["mhx_bbit_pack_dev_typed", "mhx_jaccard_topk_dev"]
    assert called_in("check(ctx.lib.mhx_jaccard_topk_dev(ctx.handle", "mhx_jaccard_topk_dev")
    assert called_in("ctx.lsh_forest_build_dev(d_sig.ptr", "mhx_lsh_forest_build_dev_typed")
    assert not called_in("# mhx_jaccard_topk_dev is described here\nctx.bbit_jaccard_topk_dev(", "mhx_jaccard_topk_dev")
    assert missing_symbols(text, "lib.mhx_jaccard_topk_dev(") == ["mhx_bbit_pack_dev_typed"]
    # a wrapper in the table is stood for by its target
    assert missing_symbols("MHX_API int mhx_bbit_pack_dev(mhx_ctx *ctx);\n", "") == ["mhx_bbit_pack_dev_typed"]
    assert missing_symbols("MHX_API int mhx_bbit_pack_dev(mhx_ctx *ctx);\n", "lib.mhx_bbit_pack_dev_typed(") == []


def test_every_device_entry_point_has_a_guard_case():
    header = _read(HEADER)
    symbols = declared_symbols(header)
    assert len(symbols) > 50 and "mhx_minhash_bulk_dev" in symbols and "mhx_ctx_device_info" not in symbols
    scripts = guard_scripts()
    assert os.path.join(ROOT, "tests", "guard_cases.py") in scripts
    text = "\n".join(_read(p) for p in scripts)
    missing = missing_symbols(header, text)
    assert not missing, (f"{len(missing)} device entry points of include/mhx.h are called in no tests/*guard_cases.py and stand in no exemption "
                         f"of tests/test_guard_ledger.py: " + ", ".join(missing))


def test_the_exemptions_are_declared_and_the_wrappers_still_forward():
    symbols = set(declared_symbols(_read(HEADER)))
    api = _read(API)
    for symbol, (target, reason) in sorted(EXEMPT.items()):
        assert reason, symbol
        assert symbol in symbols, f"{symbol} stands in the exemption table but include/mhx.h no longer declares it"
        if target is None:
            assert symbol.startswith("mhx_comm_"), f"{symbol}: only the communicator's entry points go without a guard case"
            continue
        assert target in symbols and target not in EXEMPT, (symbol, target)
        assert forwards_to(api, symbol) == target, f"{symbol} is no longer a single forwarding return to {target} in mhx_api.hip"
