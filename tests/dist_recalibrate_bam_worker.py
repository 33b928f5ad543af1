"""Launched by tests/test_gpu_recalibrate_bam.py under torch.distributed.run: `kbbq recalibrate -b ALN --kmers` in a process group.
The group is joined first, so that the function meets a group that exists (its refusal is caught and shown), then the command
line runs as a rank's would and its ValueError ends the process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'kbbq-py_amd'))

from kbbq import main, parallel, recalibrate   # noqa: E402

if __name__ == '__main__':
    sam, out, grp = sys.argv[1:4]
    parallel.init_from_env()
    import torch.distributed as dist
    print('group: initialised=%s world=%d' % (dist.is_initialized(), dist.get_world_size()), flush=True)
    try:
        recalibrate.recalibrate_bam(sam, kmers=dict(k=15), gatkreport=grp, output=out)
    except ValueError as exc:
        print('function: %s' % exc, flush=True)
    main.main(['recalibrate', '-b', sam, '--kmers', '-k', '15', '-g', grp, '-o', out])
