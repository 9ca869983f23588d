"""Seeded GTF inputs for the differential fuzz of tests/test_gtf_gpu.py (helper, not collected), in the style of
tests/fuzz_records.py: a few hundred lines per seed — valid Ensembl-shaped lines, comment lines, CRLF, bytes >= 0x80 — and, for
the odd seeds, one mutated line (a field dropped, emptied or replaced by a byte that is wrong for it), so that the first error,
its row and its offset are compared as well as the rows.  attribute_fields(seed): ninth fields alone, valid and mutated, for
exg_gtf_attributes."""
import gtf_files as G

BAD_BYTES = [b"", b"+", b"x", b"0", b"-1", b"1e", b"..", b"\xe9", b"\xc3\xa9", b"3", b"++", b" "]


def scan_input(seed, n_lines=300):
    rng = G.rng(1000 + seed)
    lines = []
    for i in range(n_lines):
        r = rng.random()
        if r < 0.08:
            lines.append(rng.choice((b"#", b"#!genome-build GRCh38", b"## a comment with\ttabs\t\t\t\t\t\t\t\tin it", b"#caf\xc3\xa9")))
        elif r < 0.12:
            lines.append(G.line(rng, seqname=rng.choice((b"chr\xc3\xa9", b"s" * rng.randrange(1, 40)))))
        elif r < 0.15:
            lines.append(G.line(rng, attrs=b'note "' + b"; " * rng.randrange(0, 900) + b'";'))
        else:
            lines.append(G.line(rng))
    if seed % 2:
        k = rng.randrange(n_lines)
        f = G.line(rng).split(b"\t")
        what = rng.randrange(3)
        if what == 0:
            f = f[:rng.randrange(0, 9)]
        else:
            f[rng.randrange(0, 8)] = rng.choice(BAD_BYTES)
        lines[k] = b"\t".join(f)
    sep = [b"\r\n" if rng.random() < 0.05 else b"\n" for _ in lines]
    data = b"".join(ln + s for ln, s in zip(lines, sep))
    return data if rng.random() < 0.5 else data[:-len(sep[-1])]


def attribute_fields(seed, n_rows=300):
    rng = G.rng(2000 + seed)
    pieces = [b" ", b";", b'"', b"k", b"key", b"v1", b"  ", b'"a b"', b'"x;y"', b'""', b"gene_id", b"\t", b"\xc3\xa9"]
    rows = []
    for i in range(n_rows):
        r = rng.random()
        if r < 0.5:
            rows.append(G.attributes(rng))
        elif r < 0.6:
            rows.append(G.attributes(rng, n_entries=8, tags=rng.randrange(0, 80)))
        else:
            rows.append(b"".join(rng.choice(pieces) for _ in range(rng.randrange(0, 40))))
    return rows
