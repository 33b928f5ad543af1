"""Launched by tests/test_gpu_bqsr_kmers.py under torch.distributed.run: `kbbq bqsr --kmers` in a process group.  The command's
ValueError is caught once to show that the context still works afterwards (the k-mer flags of the same alignments, which ask
for no group), and raised again: the process ends as the command line does."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'kbbq-py_amd'))

import numpy as np   # noqa: E402

from kbbq import main   # noqa: E402

if __name__ == '__main__':
    sam, k = sys.argv[1], int(sys.argv[2])
    try:
        main.main(['bqsr', '-b', sam, '--kmers', '-k', str(k), '-g', sys.argv[3]])
    except ValueError as exc:
        import torch
        import torch.distributed as dist
        from kbbq import aln, fastx, kmer
        print('group: initialised=%s world=%d' % (dist.is_initialized(), dist.get_world_size()), flush=True)
        b = aln.AlignmentFile(sam).batch()
        pitch = fastx.pitch_for(int(b.qlen.max()))
        seq = torch.from_numpy(b.plane(0, pitch)).cuda()
        meta = torch.from_numpy(b.qlen.astype(np.int32)).cuda()
        table = kmer.count_kmers(seq, meta, k=k)
        t = kmer.solid_threshold(kmer.kmer_histogram(table))
        flags, changed = kmer.flag_errors(table, seq, meta, t)
        print('afterwards: min_count=%d flagged_bases=%d' % (t, int(changed.sum())), flush=True)
        table.close()
        raise
