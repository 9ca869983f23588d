"""The DEFLATE writer of tests/deflate_frames.py proved against zlib's decoder before it judges the device: every catalogue
stream and generator seed inflates under zlib to exactly what the tokens describe (expected_output) and ends where the writer
says it does, zlib refuses every invalid stream, the catalogue reaches every form the list names, and the generator's own
token lists hold enough long codes in every pairing."""
import zlib

import pytest

import deflate_frames as df

SEEDS = list(range(12))
SEED_BYTES = 60_000


def zlib_inflate(raw):
    """-> (output, compressed bytes consumed) or raises zlib.error; a stream cut short raises EOFError"""
    d = zlib.decompressobj(-15)
    out = d.decompress(raw)
    if not d.eof:
        raise EOFError("the stream ends before its final block")
    return out, len(raw) - len(d.unused_data)


@pytest.mark.parametrize("name", sorted(df.catalogue()))
def test_catalogue_stream_decodes_to_expected(name):
    spec = df.catalogue()[name]
    out, used = zlib_inflate(df.encode(spec))
    assert out == df.expected_output(spec), name
    assert used == df.consumed(spec) == len(df.encode(spec)) - len(spec.trailing)


def test_generator_seeds_decode_to_expected():
    for seed in SEEDS:
        s = df.random_stream(seed, SEED_BYTES)
        raw = df.encode(s)
        out, used = zlib_inflate(raw)
        want = df.expected_output(s)
        assert want == s._content, seed          # the generator's own content: the tokens it drew regenerate it
        assert out == want and used == len(raw), seed


def test_invalid_streams_are_refused():
    inv = df.invalid()
    assert sum(n.startswith("truncated_at_") for n in inv) == len(df.encode(df.truncation_stream())) >= 300
    for name, (spec, clause, klass) in inv.items():
        raw = df.encode(spec)
        refused = False
        try:
            zlib_inflate(raw)
        except EOFError:
            refused = True
            assert klass == 5, (name, "zlib only runs out of input")
        except zlib.error:
            refused = True
            assert klass != 5, name
        assert refused != (name in df.ZLIB_ACCEPTS), (name, clause)


def test_catalogue_covers_every_form():
    seen = set()
    for spec in df.catalogue().values():
        seen |= df.forms(spec)
    assert seen == df.REQUIRED_FORMS, (sorted(df.REQUIRED_FORMS - seen), sorted(seen - df.REQUIRED_FORMS))
    # HCLEN = 4 cannot be valid (no length but 0 can be sent): it is an invalid() entry
    assert "hdr:hclen4" in df.forms(df.invalid()["hclen_4_no_lengths"][0])


def test_generator_reaches_long_codes_in_every_pairing():
    """from the generator's own token lists, no decoder involved: each pairing of a short (<= 9 bits) / long (>= 11 bits) length
    code with a short / long distance code occurs >= 1000 times over the seeds, and in the blocks that skew their codes the
    wrong way round at least a quarter of the tokens carry a long code"""
    pairs = {(a, b): 0 for a in (False, True) for b in (False, True)}
    skewed_tokens = skewed_long = 0
    seen = set()
    for seed in SEEDS:
        info = df.stats(df.random_stream(seed, SEED_BYTES))
        seen |= info["forms"]
        for lc, dc in info["pairs"]:
            if (lc >= df.LONG or lc <= df.SHORT) and (dc >= df.LONG or dc <= df.SHORT):
                pairs[(lc >= df.LONG, dc >= df.LONG)] += 1
        for mode, n_tok, n_long in info["dynamic"]:
            if mode is not None and any(mode):
                skewed_tokens += n_tok
                skewed_long += n_long
    assert min(pairs.values()) >= 1000, pairs
    assert skewed_tokens > 10_000 and 4 * skewed_long >= skewed_tokens, (skewed_long, skewed_tokens)
    assert {"tok:long_back_to_back", "tok:long_before_eob", "tok:long_first", "hdr:single_dist_code", "hdr:hdist1_len0",
            "stored:len0", "tok:258_as_284_31", "hdr:hlit286", "hdr:hdist30"} <= seen, sorted(seen)


def test_tokeniser_round_trips():
    text = b"".join(b"@read%d\nACGTACGTTTGACCA%s\n+\nIIIIFFFF##II:::\n" % (k, b"ACGT"[k % 4:]) for k in range(300))
    tokens = df.tokenise(text)
    assert df.expected_output([df.Fixed(tokens)]) == text
    assert sum(not isinstance(t, int) for t in tokens) > 300        # it does find matches
    assert zlib_inflate(df.encode(df.Stream([df.Fixed(tokens, final=True)])))[0] == text
