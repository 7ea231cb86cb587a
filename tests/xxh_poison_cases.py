"""The xxHash cases of tests/xxh_guard_cases.py on poisoned scratch and allocations (test infrastructure, run as a script in a
process of its own by tests/test_gpu_xxh_guard.py).

    python tests/xxh_poison_cases.py <byte>        prints "XXH POISON OK <n> cases (byte 0x..)" and exits 0

<byte> 0 .. 255 goes to mhx_debug_poison_alloc before the first allocation of the process, so that every fresh allocation of the
library holds nothing but that byte; guard pages stay off.  mhx_ctx_release_scratch runs before every case: the staging buffers of
a host form hold the byte, not what the case before left there -- as tests/shingle_poison_cases.py does for the SHA-1 family.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import _native  # noqa: E402
from tests import guard_cases as G  # noqa: E402
from tests import xxh_guard_cases as X  # noqa: E402


def main():
    byte = int(sys.argv[1], 0)
    _native.poison_alloc(byte)  # before the first allocation of the process
    ctx = _native.context()
    probe = ctx.alloc(100)
    assert probe.download(100, "uint8").tolist() == [byte] * 100, "the poison switch did not take effect"
    G.BETWEEN = lambda name: (print("ok", name, flush=True), ctx.release_scratch())
    ctx.release_scratch()
    X.cases(ctx)
    ctx.synchronize()
    if G.FAILED:
        print(f"XXH POISON FAILED: {G.FAILED} mismatching cases of {G.CASES}", flush=True)
        sys.exit(1)
    print(f"XXH POISON OK {G.CASES} cases (byte 0x{byte:02x})", flush=True)


if __name__ == "__main__":
    main()
