"""bzip2 inputs at the reader's door, on a box without a GPU: compression='bzip2' is accepted (the reader goes on to look
for a device and fails loudly there — no CPU fallback), while xz is still refused as unsupported."""
import bz2

import pytest


def _no_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")


@pytest.fixture()
def fastq_bz2(tmp_path):
    p = tmp_path / "reads.fastq.bz2"
    p.write_bytes(bz2.compress(b"@r1\nACGT\n+\nIIII\n@r2\nGG\n+\nII\n", 9))
    return p


@pytest.mark.parametrize("name", ["bzip2", "BZ2", "bz2", "BZIP2"])
def test_bzip2_is_accepted_and_reaches_the_device_check(fastq_bz2, name):
    _no_gpu()
    from exon_duckdb_amd import ExgError, abi
    from exon_duckdb_amd.reader import ShardReader

    with pytest.raises(ExgError) as e:
        ShardReader(str(fastq_bz2), "fastq", compression=name)
    assert e.value.code == abi.EXG_E_NO_DEVICE, str(e.value)


def test_xz_is_still_unsupported_and_named(tmp_path):
    _no_gpu()
    from exon_duckdb_amd import ExgError, abi
    from exon_duckdb_amd.reader import ShardReader

    p = tmp_path / "reads.fastq.xz"
    p.write_bytes(b"\xfd7zXZ\x00" + b"\x00" * 32)
    with pytest.raises(ExgError) as e:
        ShardReader(str(p), "fastq", compression="xz")
    assert e.value.code == abi.EXG_E_UNSUPPORTED
    assert "xz" in str(e.value) and "bzip2 / xz" not in str(e.value)


def test_bzip2_decode_is_declared_in_the_c_abi():
    from exon_duckdb_amd import abi

    assert "exg_bzip2_decode" in abi.SIGNATURES
    assert abi.EXG_ABI_VERSION == 9
