"""
The rule of static quantized qualities (--static-quantized-quals, --round-down-quantized) in plain Python integers: the
executable form of the statement in include/kbbq_hip.h ("Static quantized qualities"), written independently of
kbbq.gatk.applybqsr.quantize_map -- a loop over the 256 bytes, no NumPy.

    levels   a non-empty set of integers minscore <= Q <= 93; E = sorted({minscore} | levels)
    byte b, q = b - 33:
        b < 33 + minscore       b
        q >= E[-1]              E[-1] + 33
        E[i] <= q < E[i + 1]    E[i] + 33 if 2q <= E[i] + E[i + 1] else E[i + 1] + 33; with round_down: E[i] + 33
"""
MINSCORE = 6
TOP = 93


def check_levels(levels, minscore=MINSCORE):
    levels = list(levels)
    if not levels:
        raise ValueError('no levels')
    for q in levels:
        if type(q) is not int:
            raise ValueError('level %r is not an integer' % (q,))
        if q < minscore or q > TOP:
            raise ValueError('level %d out of range' % q)
    return sorted(set(levels) | {minscore})


def model_map(levels, round_down=False, minscore=MINSCORE):
    """The map as a list of 256 ints."""
    E = check_levels(levels, minscore)
    out = []
    for b in range(256):
        q = b - 33
        if b < 33 + minscore:
            out.append(b)
            continue
        if q >= E[-1]:
            out.append(E[-1] + 33)
            continue
        i = 0
        while not (E[i] <= q < E[i + 1]):
            i += 1
        if round_down or 2 * q <= E[i] + E[i + 1]:
            out.append(E[i] + 33)
        else:
            out.append(E[i + 1] + 33)
    return out


def map_bytes(data, table):
    """bytes -> bytes through the table."""
    return bytes(table[b] for b in data)


def map_quality_fields(text, table, field):
    """SAM or FASTQ text (bytes) with the quality field of every record passed through the table.
    field='sam': column 11 of every line that is not a header line; field='fastq': every fourth line."""
    lines = text.split(b'\n')
    out = []
    for k, line in enumerate(lines):
        if field == 'sam':
            if line and not line.startswith(b'@'):
                cols = line.split(b'\t')
                cols[10] = map_bytes(cols[10], table)
                line = b'\t'.join(cols)
        elif k % 4 == 3:
            line = map_bytes(line, table)
        out.append(line)
    return b'\n'.join(out)
