"""The legs that pass through next_batch (exg_rd_batch.cpp, exg_rd_rows_out.cpp, exg_rd_bam.cpp), for an A/B of two builds of libexon_gpu.so inside one session on one
box (profiles/next_batch_refactor_ab.md).  `make`: the inputs, once, into /dev/shm/exg_ab.  `measure LABEL`: one process = one
library (whatever exon_duckdb_amd/lib/libexon_gpu.so is at that moment): every leg once to warm, then RUNS (5) timed; prints ms.
The caller copies the variants over libexon_gpu.so in turn (as tools/ab_zst.sh does) and removes /dev/shm/exg_ab at the end."""
import os, struct, sys, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the BAM / SAM / GTF writers of the tests
import torch  # noqa: E402
import bench  # noqa: E402
from exon_duckdb_amd import device, load_library  # noqa: E402

D = "/dev/shm/exg_ab"
FQ, VCF, FA, FQGZ, VCFGZ = D + "/a.fastq", D + "/a.vcf", D + "/a.fasta", D + "/a.fastq.gz", D + "/b.vcf.gz"
BAM, SAM, GTF = D + "/a.bam", D + "/a.sam", D + "/a.gtf"


def make_rows_out_inputs():
    """BAM (400 MB decoded), SAM and GTF text (300 MB each): a block of the test writers' records, repeated"""
    import bam_files, gtf_files, sam_files
    refs = [(b"chr%d" % i, 250_000_000) for i in range(1, 23)]
    run = b"".join(bam_files.illumina_pairs(10_000, refs, seed=5))
    bam_files.write_repeated(BAM, bam_files.header(refs), run, int(4e8) // len(run))
    for path, head, block in ((SAM, sam_files.header(), sam_files.mixed(sam_files.rng(5), 20_000, read_len=150)),
                              (GTF, b"", gtf_files.mixed(gtf_files.rng(5), 20_000))):
        with open(path, "wb") as f:
            f.write(head)
            for _ in range(int(3e8) // len(block)):
                f.write(block)


def make():
    os.makedirs(D, exist_ok=True)
    n = int(4e9) // 332 * 332
    bench.write_device_bytes(torch, device.synth_fastq(n)[:n], n, FQ)
    t, nv = device.synth_vcf(40_000_000)
    bench.write_device_bytes(torch, t, nv, VCF)
    del t
    d, nf = device.synth_fasta(int(2e9 / 1712))
    bench.write_device_bytes(torch, d, nf, FA)
    del d
    # BGZF FASTQ: one block of members, repeated (tools/gz_chunks_probe.py)
    raw = device.synth_fastq(332 * 100_000)[: 332 * 100_000].cpu().numpy().tobytes()
    parts = []
    for i in range(0, len(raw), 65280):
        chunk = raw[i:i + 65280]
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        z = co.compress(chunk) + co.flush()
        parts.append(b"\x1f\x8b\x08\x04" + b"\0" * 4 + b"\0\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(z) + 8 - 1)
                     + z + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    block = b"".join(parts)
    with open(FQGZ, "wb") as f:
        for _ in range(max(1, int(1.5e9 / len(block)))):
            f.write(block)
    # a bgzip VCF of 10 M lines
    t, nv2 = device.synth_vcf(10_000_000)
    bench.write_device_bytes(torch, t, nv2, D + "/b.vcf")
    del t
    from exon_duckdb_amd.testing.bgzf import bgzip
    bgzip(D + "/b.vcf", VCFGZ)
    os.unlink(D + "/b.vcf")
    make_rows_out_inputs()
    print("inputs:", {p: os.path.getsize(os.path.join(D, p)) for p in os.listdir(D)}, flush=True)


def arrow(path, fmt):
    from exon_duckdb_amd.arrow import new_reader
    t0 = time.perf_counter()
    rows = sum(b.num_rows for b in new_reader(path, fmt))
    return rows, time.perf_counter() - t0


def measure(label):
    lib = load_library()
    runs = int(os.environ.get("RUNS", "5"))
    legs = [
        ("fastq COUNT(*)", lambda: bench.reader_count(lib, FQ, "fastq")[1]),
        ("fastq all columns", lambda: bench.reader_chunks(lib, FQ, "fastq")[2]),
        ("vcf COUNT(*)", lambda: bench.reader_count(lib, VCF, "vcf")[1]),
        ("vcf all columns", lambda: bench.reader_chunks(lib, VCF, "vcf")[2]),
        ("vcf chrom,pos,ref", lambda: bench.reader_chunks(lib, VCF, "vcf", columns=0b1011)[2]),
        ("vcf filtered pos>=20000000, chrom,pos,ref", lambda: bench.reader_chunks(lib, VCF, "vcf", columns=0b1011, filters="pos>=20000000")[2]),
        ("vcf filtered COUNT(*)", lambda: bench.reader_count(lib, VCF, "vcf", filters="pos>=20000000")[1]),
        ("fasta COUNT(*)", lambda: bench.reader_count(lib, FA, "fasta")[1]),
        ("fasta all columns", lambda: bench.reader_chunks(lib, FA, "fasta")[2]),
        ("bgzf fastq COUNT(*)", lambda: bench.reader_count(lib, FQGZ, "fastq")[1]),
        ("bgzf fastq all columns", lambda: bench.reader_chunks(lib, FQGZ, "fastq")[2]),
        ("bgzf fastq name only (side buffer)", lambda: bench.reader_chunks(lib, FQGZ, "fastq", columns=0b0001)[2]),
        ("bgzf fastq -> Arrow", lambda: arrow(FQGZ, "fastq")[1]),
        ("bgzf vcf all columns", lambda: bench.reader_chunks(lib, VCFGZ, "vcf")[2]),
        ("bgzf vcf -> Arrow", lambda: arrow(VCFGZ, "vcf")[1]),
        ("bam all columns", lambda: bench.reader_chunks(lib, BAM, "bam")[2]),
        ("bam filtered flag<128, all columns", lambda: bench.reader_chunks(lib, BAM, "bam", filters="flag<128")[2]),
        ("sam all columns", lambda: bench.reader_chunks(lib, SAM, "sam")[2]),
        ("gtf all columns with attributes", lambda: bench.reader_chunks(lib, GTF, "gtf")[2]),
    ]
    for name, fn in legs:
        fn()
        ts = [fn() * 1e3 for _ in range(runs)]
        print(f"{label} | {name} | " + " ".join(f"{t:.1f}" for t in ts) + f" | best {min(ts):.1f}", flush=True)


if __name__ == "__main__":
    make() if sys.argv[1] == "make" else measure(sys.argv[2])
