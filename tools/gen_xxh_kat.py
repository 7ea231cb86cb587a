#!/usr/bin/env python3
"""tools/gen_xxh_kat.py -- write tests/golden/xxh_kat.json, the known answers of XXH32 / XXH64 (seed 0) that
tests/test_xxh_host.py holds datasketch_amd.hashfunc.xxh32_hash32 / xxh64_hash64 to.

The answers come from the installed `xxhash` package (the C library), not from this project's code.  The byte pattern is fixed
and stated in the file: byte i = (i * 131 + 7) mod 256 for i in [0, 512).  Recorded: every prefix of length 0 .. 140, and 32
slices pattern[off : off + length] at odd offsets.

    python tools/gen_xxh_kat.py            rewrites the fixture
"""
import json
import os

import xxhash

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "xxh_kat.json")

PATTERN_BYTES = 512
PREFIXES = 141


def pattern() -> bytes:
    return bytes((i * 131 + 7) % 256 for i in range(PATTERN_BYTES))


def slices():
    """32 (offset, length) pairs: odd offsets 1, 3, ... 63; lengths that walk over the stripe and tail boundaries."""
    return [(2 * i + 1, (37 * i + 5) % 301) for i in range(32)]


def main():
    data = pattern()
    doc = {
        "pattern": "byte i = (i * 131 + 7) mod 256, i in [0, %d)" % PATTERN_BYTES,
        "pattern_bytes": PATTERN_BYTES,
        "seed": 0,
        "source": "xxhash %s (libxxhash %s)" % (xxhash.VERSION, xxhash.XXHASH_VERSION),
        "prefix_xxh32": [xxhash.xxh32_intdigest(data[:n]) for n in range(PREFIXES)],
        "prefix_xxh64": [xxhash.xxh64_intdigest(data[:n]) for n in range(PREFIXES)],
        "slices": [{"offset": o, "length": n, "xxh32": xxhash.xxh32_intdigest(data[o: o + n]), "xxh64": xxhash.xxh64_intdigest(data[o: o + n])}
                   for o, n in slices()],
    }
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
