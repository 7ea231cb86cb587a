"""The ledger behind include/mhx.h's promise that tests/test_gpu_stream_order.py holds every `_dev` entry point to the enqueue,
ordering and no-retained-pointer rules: every such symbol the header declares is called in tests/stream_order_cases.py, or stands in
the guard ledger's table of exemptions (the communicator's entries need several ranks, a forwarding wrapper is stood for by its
target), and every entry the script lists as blocking by design is a declared symbol with a reason that names the synchronise.
Runs without a GPU: it reads the header, mhx_api.hip and the script.
"""
import ast
import os
import re

from tests.test_guard_ledger import API, EXEMPT, HEADER, ROOT, called_in, declared_symbols, forwards_to

SCRIPT = os.path.join(ROOT, "tests", "stream_order_cases.py")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _blocking():
    """The BLOCKING table of the script, read from its source (importing the script would load the library)."""
    for node in ast.parse(_read(SCRIPT)).body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "BLOCKING" for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError("tests/stream_order_cases.py has no BLOCKING table")


def uncovered(header_text, script_text):
    """Declared `_dev` symbols that the script does not call and no exemption stands for."""
    missing = set()
    for symbol in declared_symbols(header_text):
        target = EXEMPT[symbol][0] if symbol in EXEMPT else symbol
        if target is not None and not called_in(script_text, target):
            missing.add(target)
    return sorted(missing)


def test_every_device_entry_point_has_a_stream_order_case():
    header, script = _read(HEADER), _read(SCRIPT)
    symbols = declared_symbols(header)
    assert len(symbols) > 50 and "mhx_minhash_bulk_dev" in symbols
    missing = uncovered(header, script)
    assert not missing, (f"{len(missing)} device entry points of include/mhx.h are called nowhere in tests/stream_order_cases.py and stand in no "
                         f"exemption of tests/test_guard_ledger.py: " + ", ".join(missing))
    assert uncovered("MHX_API int mhx_made_up_dev(mhx_ctx *ctx);\n", script) == ["mhx_made_up_dev"]


def test_the_exemptions_are_the_guard_ledgers():
    symbols = set(declared_symbols(_read(HEADER)))
    api = _read(API)
    for symbol, (target, reason) in sorted(EXEMPT.items()):
        assert symbol in symbols and reason, symbol
        if target is None:
            assert symbol.startswith("mhx_comm_"), f"{symbol}: only the communicator's entry points go without a case (they need several ranks)"
        else:
            assert forwards_to(api, symbol) == target, f"{symbol} is no longer a single forwarding return to {target} in mhx_api.hip"


def test_every_blocking_entry_is_declared_and_cites_its_synchronise():
    symbols = set(declared_symbols(_read(HEADER)))
    table = _blocking()
    assert table, "an empty BLOCKING table: the read-backs of the pair counts block by design"
    script = _read(SCRIPT)
    for symbol, reason in sorted(table.items()):
        assert symbol in symbols, f"{symbol} stands in BLOCKING but include/mhx.h does not declare it"
        assert symbol not in EXEMPT and called_in(script, symbol), f"{symbol} stands in BLOCKING but has no case"
        cited = re.findall(r"(\w+\.(?:hip|h)):(\d+)", reason)
        assert cited and "hipStreamSynchronize" in reason, f"{symbol}: the reason names no hipStreamSynchronize with its file and line"
        for name, line in cited:
            text = _read(os.path.join(ROOT, "datasketch_amd", "csrc", name)).splitlines()[int(line) - 1]
            assert "hipStreamSynchronize" in text or "read_back_u64" in text, f"{symbol}: {name}:{line} is `{text.strip()}`, no synchronise"
