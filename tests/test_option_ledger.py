"""The ledger behind the promise of include/mhx.h that an option of mhx_ctx_set_option changes timings, never results: every key of the
options[] table in mhx_api.hip has a domain, and every value of a listed domain -- both ends and an inner value of a range -- a
case in tests/option_cases.py or an exclusion with its reason; every place in datasketch_amd/csrc that reads an opt_* field is
claimed by a case of that key (or stands in the table of site exemptions); every claim is true; the launcher's condition a case
restates holds for the case's shape.  tests/test_gpu_options.py runs the cases.  Runs without a GPU: it reads the sources.
"""
import glob
import os
import re

from tests import option_cases as C
from tests.test_guard_ledger import API, HEADER, ROOT

CSRC = os.path.join(ROOT, "datasketch_amd", "csrc")
TABLE_FUNCTION = "mhx_ctx_set_option"  # the table itself and its checks: no read site
# a function definition at column 0: a declarator with a name and an opening parenthesis, not a statement
_DEFINITION = re.compile(r"^(?!#|//|typedef|using|namespace|template|extern|struct|class|enum|union|static_assert)[A-Za-z_][\w\s\*&:<>,]*?\b([A-Za-z_]\w*)\s*\(")
_FIELD = re.compile(r"\bopt_([a-z0-9_]+)\b")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def option_table(api_text):
    """key -> field (without opt_) of the options[] table of mhx_ctx_set_option."""
    start = api_text.index("} options[] = {")
    block = api_text[start: api_text.index("};", start)]
    return dict(re.findall(r'\{"([a-z_.0-9]+)",\s*&mhx_ctx::opt_([a-z0-9_]+)', block))


def read_sites(sources):
    """{(field, file, enclosing function)} of every use of an opt_* field in `sources` (file name -> text): the enclosing function is
    the nearest function definition at column 0 at or above the line.  The field declarations of mhx_internal.h and the table's
    own function do not count."""
    sites = set()
    for name, text in sources.items():
        function = None
        for line in text.splitlines():
            m = _DEFINITION.match(line)
            if m and not line.rstrip().endswith(";"):
                function = m.group(1)
            if re.match(r"\s*int64_t opt_\w+ = ", line):
                continue
            for use in _FIELD.finditer(line):
                if function != TABLE_FUNCTION:
                    sites.add((use.group(1), name, function))
    return sites


def _sources():
    paths = [p for ext in ("*.hip", "*.h", "*.inc") for p in glob.glob(os.path.join(CSRC, ext))]
    return {os.path.basename(p): _read(p) for p in sorted(paths)}


def _claims(table):
    return {(table[c.key], f, fn) for c in C.CASES if c.key in table for f, fn in c.reads}


def unclaimed(table, sources):
    """Read sites no case of the site's key claims and no exemption stands for."""
    return sorted(read_sites(sources) - _claims(table) - set(C.SITE_EXEMPT))


def keys_without_case(table):
    have = {c.key for c in C.CASES} | {k if isinstance(k, str) else k[0] for k in C.EXCLUDED}
    return sorted(set(table) - have)


def header_comment(header_text):
    end = header_text.index("MHX_API int mhx_ctx_set_option")
    return header_text[header_text.rindex("/*", 0, end): end]


def test_every_key_of_the_table_has_a_domain_and_a_case_or_an_exclusion():
    table = option_table(_read(API))
    assert len(table) >= 37 and table["lsh.sort"] == "lsh_sort" and len(set(table.values())) == len(table)
    missing = keys_without_case(table)
    assert not missing, "keys of options[] in mhx_api.hip with neither a case nor an exclusion in tests/option_cases.py: " + ", ".join(missing)
    assert set(C.DOMAIN) == set(table) == set(C.DEFAULTS), sorted(set(C.DOMAIN) ^ set(table) | set(C.DEFAULTS) ^ set(table))
    assert set(c.key for c in C.CASES) | {k if isinstance(k, str) else k[0] for k in C.EXCLUDED} == set(table)
    # the ledger's own control: a key added to the table without a case is reported
    made_up = dict(table, **{"made.up": "made_up"})
    assert keys_without_case(made_up) == ["made.up"]


def test_every_value_of_a_domain_has_a_case_or_an_exclusion_with_a_reason():
    for key, dom in C.DOMAIN.items():
        assert C.DEFAULTS[key] in dom, key
        for v in C.value_needs_case(key):
            assert v in dom, (key, v)
            cased = any(c.key == key and c.value == v for c in C.CASES)
            excluded = C.EXCLUDED.get((key, v)) or C.EXCLUDED.get(key)
            assert cased or excluded, f"{key} = {v} has neither a case nor an exclusion"
            assert not (cased and excluded), f"{key} = {v} is excluded and has a case"
        if isinstance(dom, C.Range):
            assert dom.lo < dom.inner < dom.hi and dom.inner in dom, key
        for v in C.outside(key):
            assert v not in dom, (key, v)
    for what, reason in C.EXCLUDED.items():
        key = what if isinstance(what, str) else what[0]
        assert key in C.DOMAIN and len(reason) > 20, what
        if not isinstance(what, str):
            assert what[1] in C.DOMAIN[key] and what[1] != C.DEFAULTS[key], what
    for c in C.CASES:
        assert c.value in C.DOMAIN[c.key] and c.value != C.DEFAULTS[c.key], c.id
        assert c.op in C._BUILDERS and c.reference, c.id
    assert len({c.id for c in C.CASES}) == len(C.CASES)


def test_every_place_that_reads_an_option_is_claimed_by_a_case_of_its_key():
    table = option_table(_read(API))
    sources = _sources()
    sites = read_sites(sources)
    assert len(sites) > 40 and ("minhash_p3", "minhash_kernels.hip", "launch_p") in sites and ("lsh_chunk", "lsh_kernels.hip", "scatter_rows") in sites
    assert {field for field, _, _ in sites} <= set(table.values())
    missing = unclaimed(table, sources)
    assert not missing, "option reads that no case of tests/option_cases.py claims and no SITE_EXEMPT entry stands for: " + ", ".join(map(str, missing))
    # every claim and every exemption is a real read site
    for claim in sorted(_claims(table)):
        assert claim in sites, f"a case claims {claim}, where the field is not read"
    for site, reason in C.SITE_EXEMPT.items():
        assert site in sites and len(reason) > 20, site
        assert site not in _claims(table), f"{site} is exempt and claimed"
    # the ledger's own control: a read added to a launcher no case claims is reported
    made_up = dict(sources)
    made_up["made_up_kernels.hip"] = "int launch_made_up(mhx_ctx *ctx) {\n    return ctx->opt_lsh_chunk == 8 ? 1 : 0;\n}\n"
    assert unclaimed(table, made_up) == [("lsh_chunk", "made_up_kernels.hip", "launch_made_up")]


def test_every_key_stands_in_quotes_in_the_comment_of_the_header():
    comment = header_comment(_read(HEADER))
    assert "Tuning / test knobs" in comment
    for key in option_table(_read(API)):
        assert f'"{key}"' in comment, f'include/mhx.h does not describe "{key}" in its comment on mhx_ctx_set_option'
    assert str(C.MAX_BLOCKS_PER_CU) in comment, "the bound of blocks_per_cu"
    assert '"made.up"' not in comment


def test_the_library_table_states_the_same_domains():
    """The domain table of mhx_api.hip, entry by entry, against DOMAIN: the listed values or the [lo, hi] of a range."""
    api = _read(API)
    start = api.index("} options[] = {")
    block = api[start: api.index("};", start)]
    named = {"kFlag": (0, 1), "kThree": (0, 1, 2)}
    consts = {"kAny": C.I64_MAX, "-kAny - 1": C.I64_MIN}
    for key, rest in re.findall(r'\{"([a-z_.0-9]+)",\s*&mhx_ctx::opt_\w+,\s*(.*?)\},?\s*(?://.*)?$', block, flags=re.M):
        dom = C.DOMAIN[key]
        if rest in named:
            assert dom == named[rest], key
            continue
        m = re.fullmatch(r"\{(\d+), \{([^}]*)\}, (.+?), (.+?), (\d+), (.+?)\}?", rest)
        assert m, (key, rest)
        if int(m.group(1)):
            assert dom == tuple(int(v) for v in m.group(2).split(",")), key
        elif key in ("blocks_per_cu", "debug.cus"):
            assert m.group(6) == "nullptr" and isinstance(dom, C.Range) and dom.lo == 0, key
        else:
            lo, hi = (consts[t] if t in consts else int(t) for t in (m.group(3), m.group(4)))
            assert isinstance(dom, C.Range) and (dom.lo, dom.hi, dom.step) == (lo, hi, int(m.group(5))), key
    assert "(int64_t)0xFFFFFFFFll / (512 * (int64_t)std::max(1, ctx->hw_cus))" in api and C.MAX_BLOCKS_PER_CU == 0xFFFFFFFF // (512 * 256)


def test_the_restated_conditions_hold_for_every_case_and_fail_where_the_rule_says_so():
    for c in C.CASES:
        assert c.applies(), f"{c.id}: the launcher does not read {c.key} at this shape"
    by_key = {}
    for c in C.CASES:
        by_key.setdefault((c.key, c.op), c)
    mh = lambda key, **shape: by_key[(key, "minhash")].applies(dict(C._mh(shape.pop("num_perm")), cus=0, **shape))  # noqa: E731
    # minhash.p3: three per lane is the choice at 129 .. 192 and 257 .. 384 (uint64 tokens: four from 193 on), nowhere else
    assert [k for k in (64, 128, 129, 144, 192, 193, 208, 256, 257, 300, 384, 385) if mh("minhash.p3", num_perm=k)] == [129, 144, 192, 257, 300, 384]
    assert [k for k in (128, 160, 208, 300, 513, 576, 577) if mh("minhash.p3", num_perm=k, tok="u32")] == [160, 300, 513, 576]
    # minhash.share: a last slot of at most 32 permutations in one pass: 129 .. 160, and 193 .. 224 with four per lane (uint64 tokens)
    assert [k for k in (128, 129, 160, 161, 192, 193, 224, 225, 300) if mh("minhash.share", num_perm=k)] == [129, 160, 193, 224]
    assert [k for k in (129, 160, 161, 208) if mh("minhash.share", num_perm=k, tok="u32")] == [129, 160]
    # minhash.packed: 1 matters up to 96 permutations, 2 from 97 to 128
    packed = lambda k, v: by_key[("minhash.packed", "minhash")].applies(dict(C._mh(k), cus=0), v)  # noqa: E731
    assert [k for k in (64, 96, 97, 128, 129) if packed(k, 1)] == [64, 96] and [k for k in (64, 96, 97, 128, 129) if packed(k, 2)] == [97, 128]
    # minhash.prefetch: 0 matters for CSR sets and fixed lengths below 256, 2 from 256 on
    pf = lambda v, **s: by_key[("minhash.prefetch", "minhash")].applies(dict(C._mh(128, **s), cus=1), v)  # noqa: E731
    assert pf(0) and pf(0, layout="fixed", fixed_len=255, n_sets=67) and not pf(0, layout="fixed", fixed_len=256, n_sets=67)
    assert not pf(2) and not pf(2, layout="fixed", fixed_len=255, n_sets=67) and pf(2, layout="fixed", fixed_len=256, n_sets=67)
    # a few hundred sets of 256 tokens on the whole device are split over waves: no wave per set, nothing for p3 to choose
    assert C.minhash_split(dict(C._mh(144, layout="fixed", fixed_len=256), cus=0)) and not mh("minhash.p3", num_perm=144, layout="fixed", fixed_len=256)
    # the LSH sort: the options of the radix path take the bucketing away; fewer than four bins leave nothing for levels / bigbins
    ls = lambda key, **s: by_key[(key, "lsh_sort")].applies(dict(C._ls(s.pop("source", "band_major"), **s), cus=s.get("cus", 0)))  # noqa: E731
    assert ls("lsh.levels") and not ls("lsh.levels", n=5001) and ls("lsh.bigbins") and not ls("lsh.bigbins", n=5001)
    assert ls("lsh.chunk") and ls("lsh.chunk", source="row_major") and not ls("lsh.chunk", source="row_major", bands=6)
    assert not ls("lsh.prehash") and not ls("lsh.prehash", source="signatures", bands=6)
    team = by_key[("lsh.team", "lsh_sort")]
    assert team.applies(dict(C._ls("band_major"), cus=0), 1024) and not team.applies(dict(C._ls("band_major"), cus=0), 256)
    assert team.applies(dict(C._ls("band_major", bands=8), cus=1), 256) and not team.applies(dict(C._ls("band_major", bands=8), cus=1), 1024)
    # weighted: the kernels of tests/weighted_dispatch.py
    wk = lambda key, v, *a, **s: by_key[(key, "weighted")].applies(dict(C._wm(*a, **s), cus=0), v)  # noqa: E731
    assert wk("weighted.kernel", 1, 64, 64) and not wk("weighted.kernel", 1, 62, 64) and not wk("weighted.kernel", 2, 62, 64)
    assert wk("weighted.refill", 13, 64, 128) and not wk("weighted.refill", 13, 64, 64) and not wk("weighted.refill", 2, 64, 128)
    assert wk("weighted.min_dim", 64, 32, 64) and not wk("weighted.min_dim", 64, 64, 64) and not wk("weighted.min_dim", 64, 30, 64)
    assert wk("weighted.rescue", 1, 64, 64) and not wk("weighted.rescue", 1, 62, 64) and not wk("weighted.rescue", 1, 64, 128)
    assert wk("weighted.split", 1, 1022, 128) and not wk("weighted.split", 1, 1024, 128) and not wk("weighted.split", 1, 1022, 128, densities=(0.3, 1.0))
    assert wk("weighted.direct", 500, 200, 64) and not wk("weighted.direct", 500, 200, 64, densities=(0.02, 1.0))
    # the rest
    assert not by_key[("jaccard.topk_path", "topk")].applies(dict(rows="bbit", m=3, n=300, k_perm=64, k=10, cus=0), 1)
    assert not by_key[("jaccard.topk_path", "topk")].applies(dict(rows="dense", m=130, n=300, k_perm=64, k=10, cus=0), 1)
    assert not by_key[("jaccard.topk_segments", "topk")].applies(dict(rows="dense", m=3, n=128, k_perm=64, k=10, cus=0))
    assert not by_key[("overlap.bins", "overlap")].applies(dict(tiny=8, mid=8, top=8, n_pairs=400, dtype="u32", cus=0))
    assert not by_key[("hll.split_tokens", "hll")].applies(dict(p=4, n_sets=67, long=5000, dtype="u32", cus=0), C.I64_MAX)
    assert not by_key[("lsh.merge_items", "lsh_merge")].applies(dict(bands=3, n_a=1000, n_b=1000, cus=0), 8)
    assert not by_key[("pack.fused", "pack_digests")].applies(dict(n=517, num_perm=100, bands=10, r=10, b=4, dtype="u32", cus=0))
    assert not by_key[("host.chunk_bytes", "minhash_host")].applies(dict(C._mh(128, layout="fixed", fixed_len=100), cus=0), 1 << 20)
