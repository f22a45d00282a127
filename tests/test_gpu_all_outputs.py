"""Every output of worker_iterator switched on at once against each switched on alone, on the GPU, through the three work loops
(batched, ISS_ITEMWISE=1, rng="mt"): the readers of a generate call -- --report, --error_report, --depth, --origins, and the reads
as FASTQ, uBAM or with --bgzip text -- must not disturb one another, whatever order the loop runs them in.  What each file has to
hold is pinned by the feature's own tests (test_gpu_tally, test_gpu_errtally, test_gpu_depth, test_gpu_origins, test_gpu_ubam,
test_gpu_bgzf_text, test_gpu_vcf); here the files of the runs are compared with one another, byte for byte.

Three records -- 3 000 and 5 000 random bases and one of 100, shorter than the NovaSeq model's reads -- 200 pairs over the three
work items, 64 pairs a batch: the batches are cut across the items (64 | 26 + 38 | 64 | 8) and a record spans two batches."""
import gzip
import os

import numpy as np
import pytest
import torch  # noqa: F401  (when the module is collected: torch's HIP runtime has to be the process's first, see test_gpu_tensors.py)

import helpers as H

pytestmark = pytest.mark.gpu

LOOPS = ("batched", "itemwise", "mt")
FLAGS = ("report", "error_report", "depth", "origins")
CPU, SEED = 3, 11


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """run(loop, *flags) -> {file name less the prefix: its bytes} of one worker_iterator call; every distinct call is made once."""
    from insilicoseq_amd import generator as G

    dense = H.dense_model("novaseq")
    dense.store_mutations = True
    assert dense.read_length > 100
    records = [G.Record(H.random_genome(41, 3000), id="first"), G.Record(H.random_genome(42, 100), id="short"),
               G.Record(H.random_genome(43, 5000), id="second.1")]
    work = [(records[0], 90, "default"), (records[1], 10, "default"), (records[2], 110, "default")]
    done = {}

    def run(loop, *flags):
        key = (loop,) + tuple(sorted(flags))
        if key not in done:
            folder = tmp_path_factory.mktemp("_".join(key))
            with pytest.MonkeyPatch.context() as mp:
                mp.setattr(G.Worker, "BATCH_PAIRS", 64)
                for name in ("ISS_HOST_FASTQ", "ISS_HOST_VCF", "ISS_ITEMWISE"):
                    mp.delenv(name, raising=False)
                if loop == "itemwise":
                    mp.setenv("ISS_ITEMWISE", "1")
                G.worker_iterator(work, dense, CPU, str(folder / "w"), SEED, "metagenomics", False, device=0,
                                  rng="mt" if loop == "mt" else "philox", **{flag: True for flag in flags})
            done[key] = {name[1:]: open(str(folder / name), "rb").read() for name in sorted(os.listdir(str(folder)))}
        return done[key]

    return run


def _npz(data, tmp_path):
    path = str(tmp_path / "depth.npz")
    with open(path, "wb") as fh:
        fh.write(data)
    return dict(np.load(path))


@pytest.mark.parametrize("loop", LOOPS)
def test_every_flag_at_once_writes_what_each_alone_writes(run, loop, tmp_path):
    plain, every = run(loop), run(loop, *FLAGS)
    assert sorted(plain) == [".vcf", "_R1.fastq", "_R2.fastq"]
    assert sorted(every) == [".depth.npz", ".errtally.npy", ".tally.npy", ".vcf", "_R1.fastq", "_R2.fastq", "_origins.bedpe"]
    assert plain["_R1.fastq"].count(b"\n") == 4 * 200 and len(plain[".vcf"]) > 0
    for name in ("_R1.fastq", "_R2.fastq", ".vcf"):
        assert every[name] == plain[name], (loop, name)
    alone = {flag: run(loop, flag) for flag in FLAGS}
    for flag, files in alone.items():
        for name in ("_R1.fastq", "_R2.fastq", ".vcf"):
            assert files[name] == plain[name], (loop, flag, name)
    # (np.save of equal words is equal bytes: dtype and shape are in the header)
    assert every[".tally.npy"] == alone["report"][".tally.npy"]
    assert every[".errtally.npy"] == alone["error_report"][".errtally.npy"]
    got, want = _npz(every[".depth.npz"], tmp_path), _npz(alone["depth"][".depth.npz"], tmp_path)
    assert sorted(got) == sorted(want) == ["diff", "ordinals", "table"]
    for name in want:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (loop, name)
    assert np.abs(want["diff"]).sum() > 0
    assert every["_origins.bedpe"] == alone["origins"]["_origins.bedpe"] and every["_origins.bedpe"].count(b"\n") == 200


def test_the_loops_agree_where_they_share_the_random_numbers(run):
    """(batched and item-wise Philox are the same files; the MT worker draws other reads)"""
    a, b = run("batched", *FLAGS), run("itemwise", *FLAGS)
    assert sorted(a) == sorted(b)
    for name in a:
        if name != ".depth.npz":  # (a zip archive: compared array by array above)
            assert a[name] == b[name], name
    assert run("mt")["_R1.fastq"] != run("batched")["_R1.fastq"]


@pytest.mark.parametrize("loop", LOOPS)
def test_ubam_beside_every_flag(run, loop):
    alone, every = run(loop, "ubam"), run(loop, "ubam", *FLAGS)
    assert sorted(alone) == [".bam", ".vcf"] and len(alone[".bam"]) > 0
    assert every[".bam"] == alone[".bam"]
    assert every[".vcf"] == run(loop)[".vcf"]
    for name in (".tally.npy", ".errtally.npy", "_origins.bedpe"):
        assert every[name] == run(loop, *FLAGS)[name], (loop, name)


@pytest.mark.parametrize("loop", LOOPS)
def test_bgzip_beside_every_flag(run, loop):
    text, packed = run(loop, *FLAGS), run(loop, "bgzip", *FLAGS)
    assert sorted(packed) == sorted(text)
    for name in (".vcf", "_origins.bedpe"):
        assert packed[name][:4] == b"\x1f\x8b\x08\x04" and packed[name] != text[name]
        assert gzip.decompress(packed[name]) == text[name], (loop, name)  # (every member's CRC-32 and ISIZE verified on the way)
    for name in ("_R1.fastq", "_R2.fastq", ".tally.npy", ".errtally.npy"):
        assert packed[name] == text[name], (loop, name)
    alone = run(loop, "bgzip", "origins")
    assert alone[".vcf"] == packed[".vcf"] and alone["_origins.bedpe"] == packed["_origins.bedpe"]
