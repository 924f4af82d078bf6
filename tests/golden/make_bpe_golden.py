"""Golden vector for the BPE tokenizer test: the merges of OpenAI's CLIP vocabulary file that tokenizing the test strings applies,
with their ranks.  The file itself (bpe_simple_vocab_16e6.txt.gz, 1.3 MB of OpenAI's data) is not shipped; the test rebuilds a merges
file of the same length from this subset (the other ranks hold merges that never match), which tokenizes these strings to the same ids:
at every step the lowest-ranked pair present in the full table is applied, so it is in the subset and is the lowest-ranked there too.

    python tests/golden/make_bpe_golden.py /path/to/bpe_simple_vocab_16e6.txt.gz

bpe_merges_used.npz   ranks int32 [n], merges str [n, 2]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import TOKENIZER_STRINGS  # noqa: E402
from rlcf_amd.bpe import ClipBPE  # noqa: E402

EXTRA_STRINGS = ["word " * 100]          # the over-long input of the test (truncation)


class _Recorder(dict):
    """ClipBPE._bpe asks `best in ranks` exactly once per merge it applies"""
    def __init__(self, ranks):
        super().__init__(ranks)
        self.used = set()

    def __contains__(self, pair):
        hit = dict.__contains__(self, pair)
        if hit:
            self.used.add(pair)
        return hit


def main():
    tok = ClipBPE(sys.argv[1])
    rec = _Recorder(tok.ranks)
    tok.ranks = rec
    for s in TOKENIZER_STRINGS + EXTRA_STRINGS:
        tok.encode(s)
    used = sorted(rec.used, key=rec.get)
    np.savez(os.path.join(HERE, "bpe_merges_used.npz"), ranks=np.array([rec[m] for m in used], np.int32),
             merges=np.array(used, dtype=str))
    print(f"{len(used)} merges of {len(rec)}")


if __name__ == "__main__":
    main()
