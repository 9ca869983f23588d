"""An independent restatement of the reference's sequence scalars (exon/src/exon/sequence_functions/module.cpp:30-370) and SAM
flag predicates (rust/src/sam_functions.rs:19-90), for the tests of exg_sequence_op and of the host scalars: dictionaries and
loops, nothing shared with the library.  Plus a builder for duckdb::string_t columns (inline and pointer forms, NULL rows,
sources at chosen alignments inside a payload) and the decoder / packing check of an output column."""
import functools
import struct

import numpy as np

COMPLEMENT, REVERSE_COMPLEMENT, TRANSCRIBE, REVERSE_TRANSCRIBE, TRANSLATE, GC_CONTENT = 1, 2, 3, 4, 5, 6
STRING_OPS = (COMPLEMENT, REVERSE_COMPLEMENT, TRANSCRIBE, REVERSE_TRANSCRIBE, TRANSLATE)
ALL_OPS = STRING_OPS + (GC_CONTENT,)
OP_NAMES = {COMPLEMENT: "complement", REVERSE_COMPLEMENT: "reverse_complement", TRANSCRIBE: "transcribe",
            REVERSE_TRANSCRIBE: "reverse_transcribe", TRANSLATE: "translate_dna_to_aa", GC_CONTENT: "gc_content"}
PE_INVALID_CHARACTER, PE_LENGTH, PE_CODON = 30, 31, 32

MAPS = {
    COMPLEMENT: {"A": "T", "T": "A", "C": "G", "G": "C"},                      # module.cpp:81-121
    REVERSE_COMPLEMENT: {"A": "C", "T": "G", "C": "A", "G": "T"},              # module.cpp:30-69: the order is kept
    TRANSCRIBE: {"A": "A", "T": "U", "C": "C", "G": "G"},                      # module.cpp:215-253
    REVERSE_TRANSCRIBE: {"A": "A", "U": "T", "C": "C", "G": "G"},              # module.cpp:168-205
}
CODONS = {                                                                     # module.cpp:266-330
    "AAA": "K", "AAT": "N", "AAC": "N", "AAG": "K", "ATA": "I", "ATT": "I", "ATC": "I", "ATG": "M",
    "ACA": "T", "ACT": "T", "ACC": "T", "ACG": "T", "AGA": "R", "AGT": "S", "AGC": "S", "AGG": "R",
    "TAA": "*", "TAT": "Y", "TAC": "Y", "TAG": "*", "TTA": "L", "TTT": "F", "TTC": "F", "TTG": "L",
    "TCA": "S", "TCT": "S", "TCC": "S", "TCG": "S", "TGA": "*", "TGT": "C", "TGC": "C", "TGG": "W",
    "CAA": "Q", "CAT": "H", "CAC": "H", "CAG": "Q", "CTA": "L", "CTT": "L", "CTC": "L", "CTG": "L",
    "CCA": "P", "CCT": "P", "CCC": "P", "CCG": "P", "CGA": "R", "CGT": "R", "CGC": "R", "CGG": "R",
    "GAA": "E", "GAT": "D", "GAC": "D", "GAG": "E", "GTA": "V", "GTT": "V", "GTC": "V", "GTG": "V",
    "GCA": "A", "GCT": "A", "GCC": "A", "GCG": "A", "GGA": "G", "GGT": "G", "GGC": "G", "GGG": "G",
}
SAM_FLAGS = {"is_segmented": 0x1, "is_properly_aligned": 0x2, "is_unmapped": 0x4, "is_mate_unmapped": 0x8,
             "is_reverse_complemented": 0x10, "is_mate_reverse_complemented": 0x20, "is_first_segment": 0x40,
             "is_last_segment": 0x80, "is_secondary": 0x100, "is_quality_control_failed": 0x200, "is_duplicate": 0x400,
             "is_supplementary": 0x800}


class SeqError(Exception):
    """code = PE_*, offset = where in the row, text = the reference's exception message (bytes)"""

    def __init__(self, code, offset, length, text):
        super().__init__(text)
        self.code, self.offset, self.length, self.text = code, offset, length, text


def sam_flag(name, flag):
    return bool((flag & 0xFFFF) & SAM_FLAGS[name])      # the C++ side passes a u16


def gc_content(s):
    """-> numpy.float32: (float)count / (float)size in one float32 division, 0 for the empty string"""
    if not s:
        return np.float32(0)
    count = sum(1 for c in s if c in (ord("G"), ord("C")))
    return np.float32(count) / np.float32(len(s))


def apply(op, s):
    """one row: bytes -> bytes (string ops) / numpy.float32 (GC_CONTENT); None -> None; SeqError as the reference throws"""
    if s is None:
        return None
    if op == GC_CONTENT:
        return gc_content(s)
    if op == TRANSLATE:
        if len(s) % 3:
            raise SeqError(PE_LENGTH, 0, len(s), b"Invalid sequence length: " + str(len(s)).encode())
        out = bytearray()
        for i in range(0, len(s), 3):
            codon = s[i:i + 3]
            aa = CODONS.get(codon.decode("latin-1"))
            if aa is None:
                raise SeqError(PE_CODON, i, len(s), b"Invalid codon: " + codon)
            out += aa.encode()
        return bytes(out)
    table = {ord(k): ord(v) for k, v in MAPS[op].items()}
    out = bytearray()
    for i, c in enumerate(s):
        if c not in table:
            raise SeqError(PE_INVALID_CHARACTER, i, len(s), b"Invalid character in sequence: " + bytes([c]))
        out.append(table[c])
    return bytes(out)


@functools.lru_cache(maxsize=1 << 16)
def apply_fast(op, s):
    """apply() at the speed the GPU tests need: memoised, and numpy lookups instead of the loops for valid rows of 64 bytes
    and more (test_seqfn_host.py holds it against apply()); anything invalid goes through apply(), so the error is the loop's"""
    if s is None or len(s) < 64:
        return apply(op, s)
    a = np.frombuffer(s, np.uint8)
    if op == GC_CONTENT:
        return np.float32(int(np.count_nonzero((a == ord("G")) | (a == ord("C"))))) / np.float32(len(s))
    if op == TRANSLATE:
        if len(s) % 3:
            return apply(op, s)
        lut = np.full(256, 255, np.uint32)
        for k, c in enumerate(b"ACGT"):
            lut[c] = k
        idx = lut[a].reshape(-1, 3)
        if (idx == 255).any():
            return apply(op, s)
        table = np.zeros(64, np.uint8)
        for codon, aa in CODONS.items():
            table[sum(b"ACGT".index(ord(ch)) * w for ch, w in zip(codon, (16, 4, 1)))] = ord(aa)
        return table[idx[:, 0] * 16 + idx[:, 1] * 4 + idx[:, 2]].tobytes()
    lut = np.zeros(256, np.uint8)
    ok = np.zeros(256, bool)
    for k, v in MAPS[op].items():
        lut[ord(k)], ok[ord(k)] = ord(v), True
    if not ok[a].all():
        return apply(op, s)
    return lut[a].tobytes()


def first_error(op, rows):
    """(row index, SeqError) of the lowest failing row, or None"""
    for r, s in enumerate(rows):
        try:
            apply_fast(op, s)
        except SeqError as e:
            return r, e
    return None


# ---- duckdb::string_t columns --------------------------------------------------------------------------------------------
def build_column(rows, payload_base=1 << 40, alignments=None, slack=b"", lead=0):
    """rows: list of bytes / None -> (string_t array [n, 16] uint8, payload uint8 array).  Rows of up to 12 bytes are inlined
    (zero padded), NULL rows are 16 zero bytes, longer rows point at payload_base + offset; the k-th long row's offset is
    congruent to alignments[k % len(alignments)] mod 16 (default: whatever packing gives, after `lead` bytes); `slack` goes
    in front of every long row, and its bytes fill every gap (never zeros: bytes that no row may be seen to read)."""
    col = bytearray(16 * len(rows))
    parts, at, k = [], 0, 0
    fill = slack or b"#"

    def pad(m):
        nonlocal at
        parts.append((fill * (m // len(fill) + 1))[:m])
        at += m
    pad(lead)
    for r, s in enumerate(rows):
        if s is None:
            continue
        if len(s) <= 12:
            struct.pack_into("<I12s", col, 16 * r, len(s), s)
            continue
        if alignments is not None:
            pad((alignments[k % len(alignments)] - at) % 16)
            k += 1
        elif slack:
            pad(len(slack))
        struct.pack_into("<I4sQ", col, 16 * r, len(s), s[:4], payload_base + at)
        parts.append(s)
        at += len(s)
    pad(16)
    return np.frombuffer(bytes(col), np.uint8).reshape(len(rows), 16).copy(), np.frombuffer(b"".join(parts), np.uint8).copy()


def decode_column(col, payload, base):
    """string_t array [n, 16] uint8 + its payload -> list of bytes (a NULL row reads as b"": validity is the input's)"""
    raw, data = col.tobytes(), payload.tobytes()
    out = []
    for i in range(col.shape[0]):
        ln, = struct.unpack_from("<I", raw, 16 * i)
        if ln <= 12:
            out.append(raw[16 * i + 4:16 * i + 4 + ln])
        else:
            o = struct.unpack_from("<Q", raw, 16 * i + 8)[0] - base
            assert 0 <= o and o + ln <= len(data), f"row {i} points outside the payload"
            out.append(data[o:o + ln])
    return out


def expected_column(outputs, out_base):
    """the output contract of the string ops, from the rows' expected outputs (bytes; None = NULL): the string_t array
    byte for byte (inlined rows zero padded, long rows {length, prefix, out_base + offset}) and the payload (the long rows
    packed in row order without gaps)"""
    col = bytearray(16 * len(outputs))
    parts, at = [], 0
    for r, s in enumerate(outputs):
        if not s:
            continue
        if len(s) <= 12:
            struct.pack_into("<I12s", col, 16 * r, len(s), s)
        else:
            struct.pack_into("<I4sQ", col, 16 * r, len(s), s[:4], out_base + at)
            parts.append(s)
            at += len(s)
    return np.frombuffer(bytes(col), np.uint8).reshape(len(outputs), 16), np.frombuffer(b"".join(parts), np.uint8)
