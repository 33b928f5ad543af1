"""What `--skip-unresolved` does to a quality plane, as the tests construct it: a test helper only.

K1 leaves a base out of every table -- as an error, as an observation and as a dinucleotide context -- when the base's OWN quality
is below minscore (the reference's generic_dinuc_covariate: `quals[..., 1:] < minscore`), so a quality plane with a low byte at
the class-2 bases of the k-mer rule (tests/kmer_passes_model.py) is the tally that skips them, and nothing changes for their
neighbours.  The device writes byte 0 (the padding's byte) into its tally plane; a FASTQ file cannot hold that byte, so the file
the commands are compared on has '!' (quality 0) there."""
import numpy as np


def masked_quals(qual, cls, byte=ord('!')):
    """`qual` with `byte` at every class-2 base of `cls` (same shape), every other byte as it is."""
    qual = np.asarray(qual, dtype=np.uint8)
    cls = np.asarray(cls)
    assert qual.shape == cls.shape
    return np.where(cls == 2, np.uint8(byte), qual).astype(np.uint8)
