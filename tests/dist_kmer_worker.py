"""Launched by tests under torch.distributed.run: every rank reads its shard of a FASTQ file, counts it into its owner table
(kbbq.kmer.count_kmers_ranks) and saves the table's entries and the summed histogram to OUT.rankNNNN.npz.
Arguments: reads.fq k local_slots OUT."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'kbbq-py_amd'))

import numpy as np       # noqa: E402

from kbbq import kmer, parallel   # noqa: E402

if __name__ == '__main__':
    path, k, local_slots, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    world, rank = parallel.init_from_env()
    names, seq, qual, meta = kmer._read_shard(path, rank, world)
    table = kmer.count_kmers_ranks(seq, meta, k=k, local_slots=local_slots)
    hist = kmer.kmer_histogram_ranks(table)
    keys, counts = table.entries()
    table.close()
    np.savez('%s.rank%04d.npz' % (out, rank), keys=keys, counts=counts, hist=hist, reads=len(names))
