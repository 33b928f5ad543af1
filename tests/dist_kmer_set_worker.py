"""Launched by tests under torch.distributed.run: `kbbq correct --kmers-from SET` on every rank, through the command line's own
entry point, so that what a rank prints and how it exits is the command's.  Arguments: those of `kbbq`."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'kbbq-py_amd'))

from kbbq import main   # noqa: E402

if __name__ == '__main__':
    assert '--kmers-from' in sys.argv, 'this worker is for runs that load a k-mer set'
    main.main(sys.argv[1:])
