"""Wall time of getting a genome FASTA into HBM, host route against device route (Measured):

    host    generator.parse_fasta(path) + ReadEngine.add_genome / add_genomes
    device  fasta.read(path, device) + ReadEngine.add_genomes_fasta        (generate --device_fasta)

on two inputs -- one record of 200 M letters in 60-letter lines, and 20 000 records of 10 kbp -- in one process, three times each,
alternating.  One JSON line per run, then one with the medians.

    python tools/fasta_bench.py [--letters 200000000] [--records 20000] [--repeats 3] [--dir DIR]
    rocprofv3 --kernel-trace --stats -d prof -- python tools/fasta_bench.py --only device --repeats 1     # the kernels' times
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from insilicoseq_amd import fasta  # noqa: E402
from insilicoseq_amd.engine import ReadEngine  # noqa: E402
from insilicoseq_amd.generator import SMALL_RECORD, parse_fasta  # noqa: E402


def write_fasta(path, n_records, letters_each, width=60, seed=1):
    """``n_records`` records of ``letters_each`` random A/C/G/T in lines of ``width``."""
    rng = np.random.RandomState(seed)
    lines, last = divmod(letters_each, width)
    with open(path, "wb") as fh:
        for r in range(n_records):
            fh.write(b">record_%d some description\n" % r)
            body = np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, size=letters_each)]
            block = np.full((lines, width + 1), 10, np.uint8)
            block[:, :width] = body[:lines * width].reshape(lines, width)
            fh.write(block.tobytes())
            if last:
                fh.write(body[lines * width:].tobytes() + b"\n")


def host_route(eng, path):
    t0 = time.perf_counter()
    records = list(parse_fasta(path))
    t1 = time.perf_counter()
    small = [r.seq for r in records if len(r.seq) <= SMALL_RECORD]
    gids = eng.add_genomes(small) if small else []
    gids += [eng.add_genome(r.seq) for r in records if len(r.seq) > SMALL_RECORD]
    eng.synchronize()
    t2 = time.perf_counter()
    return {"read_s": t1 - t0, "upload_s": t2 - t1, "total_s": t2 - t0, "genomes": sum(g >= 0 for g in gids)}


def device_route(eng, path):
    t0 = time.perf_counter()
    records = fasta.read(path, device=eng.device)
    t1 = time.perf_counter()
    gids = eng.add_genomes_fasta([r.seq for r in records])
    eng.synchronize()
    t2 = time.perf_counter()
    return {"read_s": t1 - t0, "upload_s": t2 - t1, "total_s": t2 - t0, "genomes": sum(g >= 0 for g in gids)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--letters", type=int, default=200000000)
    ap.add_argument("--records", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["host", "device"], default=None)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--check", action="store_true", help="compare the resident letters of the two routes (first record of each input)")
    args = ap.parse_args()
    routes = [(name, fn) for name, fn in (("host", host_route), ("device", device_route)) if args.only in (None, name)]
    with tempfile.TemporaryDirectory(dir=args.dir) as d, ReadEngine(0) as eng:
        inputs = {"one_record": (1, args.letters), "many_records": (args.records, args.letters // args.records)}
        for shape, (n, each) in inputs.items():
            path = os.path.join(d, shape + ".fasta")
            write_fasta(path, n, each)
            runs = {name: [] for name, _fn in routes}
            for rep in range(args.repeats):
                for name, fn in routes:
                    res = fn(eng, path)
                    if args.check and rep == 0:
                        res["first_record_crc"] = zlib.crc32(eng.genome_letters(0).tobytes())
                    eng.clear_genomes()
                    runs[name].append(res)
                    print(json.dumps(dict(res, shape=shape, route=name, rep=rep, bytes=os.path.getsize(path))), flush=True)
            print(json.dumps({"shape": shape, "median_total_s": {name: statistics.median(r["total_s"] for r in rs) for name, rs in runs.items()},
                              "median_read_s": {name: statistics.median(r["read_s"] for r in rs) for name, rs in runs.items()},
                              "median_upload_s": {name: statistics.median(r["upload_s"] for r in rs) for name, rs in runs.items()}}), flush=True)
            os.remove(path)


if __name__ == "__main__":
    main()
