"""Generate tests/golden/soft_targets.npz by running the REAL reference's utils.metrics.VQAChallengeAccuracy.

Run in the build container only (the reference never travels to the GPU box):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_soft_golden.py <reference checkout>

2048 questions x 10 annotators in four blocks of 512 over 50, 100, 500 and 1000 answers.  Annotator answers are answer ids
(-1: not in the vocabulary) and predictions are ids too; the reference compares strings, so both are rendered with str().
Rows cover: no in-vocabulary answer at all, -1 entries mixed in, a leading answer with 1, 2, 3 and 4..10 votes, and predictions
that hit the leader, a minority answer, or nothing.  Stored: the ids, the predictions, the block sizes, the reference's score per
question (a fresh instance each), and total_score / count / compute() of one instance fed everything in four updates.
Only data is stored -- no reference source.
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
if len(sys.argv) != 2:
    sys.exit("usage: make_soft_golden.py <reference checkout>")
sys.path.insert(0, sys.argv[1])

from utils.metrics import VQAChallengeAccuracy  # noqa: E402  (the reference)

OUT = os.path.dirname(os.path.abspath(__file__))
BLOCK, A = 512, 10
BLOCK_N = (50, 100, 500, 1000)


def make_block(rng, n):
    ans = np.full((BLOCK, A), -1, dtype=np.int64)
    pred = np.zeros(BLOCK, dtype=np.int64)
    for q in range(BLOCK):
        kind = q % 8
        if kind == 0:                                   # nobody answered inside the vocabulary
            pred[q] = rng.integers(0, n)
            continue
        votes = (1, 2, 3, int(rng.integers(4, A + 1)), int(rng.integers(1, A + 1)), 2, 3)[kind - 1]
        lead = int(rng.integers(0, n))
        row = [lead] * votes
        while len(row) < A:                             # the rest: other answers (repeats allowed) and out-of-vocabulary entries
            row.append(-1 if rng.random() < 0.3 else int(rng.integers(0, n)))
        row = np.array(row, dtype=np.int64)
        rng.shuffle(row)
        ans[q] = row
        u = rng.random()
        if u < 0.5:
            pred[q] = lead
        elif u < 0.75:
            inv = row[row >= 0]
            pred[q] = inv[rng.integers(0, len(inv))]
        else:
            pred[q] = rng.integers(0, n)                # mostly hits nothing
    return ans, pred


def main():
    rng = np.random.default_rng(20240607)
    blocks = [make_block(rng, n) for n in BLOCK_N]
    answers = np.concatenate([b[0] for b in blocks])
    pred = np.concatenate([b[1] for b in blocks])
    as_str = lambda a: [[str(int(v)) for v in row] for row in a]
    scores = np.zeros(len(pred), dtype=np.float64)
    for q in range(len(pred)):
        m = VQAChallengeAccuracy()
        m.update([str(int(pred[q]))], as_str(answers[q:q + 1]))
        scores[q] = m.total_score
    m = VQAChallengeAccuracy()
    for b in range(len(BLOCK_N)):
        sl = slice(b * BLOCK, (b + 1) * BLOCK)
        m.update([str(int(v)) for v in pred[sl]], as_str(answers[sl]))
    hit = (answers == pred[:, None]).sum(1)
    assert (hit == 0).sum() > 100 and all((hit == v).sum() > 20 for v in (1, 2, 3)) and (hit > 3).sum() > 20
    assert ((answers >= 0).sum(1) == 0).sum() == len(pred) // 8
    np.savez_compressed(os.path.join(OUT, "soft_targets.npz"), answers=answers.astype(np.int16), pred=pred.astype(np.int16),
                        block_n=np.array(BLOCK_N, dtype=np.int64), scores=scores, total_score=np.float64(m.total_score),
                        count=np.int64(m.count), compute=np.float64(m.compute()))
    print("soft_targets.npz:", len(pred), "questions, compute() =", m.compute())


if __name__ == "__main__":
    main()
