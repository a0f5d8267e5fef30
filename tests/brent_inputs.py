"""Writes the inputs of the bin/MMchecker measurements of DESIGN.md 2.12 into a directory (not a test; nothing here is committed
as data):
    dense8_{L,R,P}.sms     the naive 8x8x8 algorithm after a random change of basis modulo 2147483629 (r = 512, rows of 64 entries)
    dense16_{L,R,P}.sms    the same for 16x16x16 (r = 4096, rows of 256 entries, 1.7e7 equations)
    wino4_{L,R,P}.sms      the fourth tensor power of Winograd's algorithm, sparse (16x16x16, r = 2401)
usage: python tests/brent_inputs.py DIR [dense8 dense16 wino4]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import brent_lib as B  # noqa: E402


def write_dense(path, A):
    A = np.asarray(A)
    with open(path, "w") as f:
        f.write("%d %d M\n" % A.shape)
        for i, j in zip(*np.nonzero(A)):
            f.write("%d %d %d\n" % (i + 1, j + 1, A[i, j]))
        f.write("0 0 0\n")


def dense_naive(s, seed):
    """change_basis of tests/brent_lib.py on arrays: the dictionaries of a 4096 x 256 matrix take too long"""
    import random
    q = B.P31
    rng = random.Random(seed)

    def draw():
        while True:
            M = [[rng.randrange(q) for _ in range(s)] for _ in range(s)]
            Mi = B.inverse_mod(M, q)
            if Mi is not None:
                return np.array(M, dtype=np.int64), np.array(Mi, dtype=np.int64)

    (U, Ui), (V, Vi), (W, Wi) = draw(), draw(), draw()
    L, R, P, _ = B.naive(s, s, s)
    kron = lambda X, Y: np.kron(X, Y) % q  # noqa: E731
    return (B.matmul_mod(B.dense_mod(L, q), kron(Ui, V), q), B.matmul_mod(B.dense_mod(R, q), kron(Vi.T, W), q), B.matmul_mod(kron(U, Wi), B.dense_mod(P, q), q))


def main():
    out = sys.argv[1]
    which = sys.argv[2:] or ["dense8", "dense16", "wino4"]
    os.makedirs(out, exist_ok=True)
    for name in which:
        if name.startswith("dense"):
            mats = dense_naive(int(name[5:]), 1)
            for x, A in zip("LRP", mats):
                write_dense(os.path.join(out, "%s_%s.sms" % (name, x)), A)
        else:
            W = B.load("2x2x2_7_Winograd")
            T = B.tensor(B.tensor(W, W), B.tensor(W, W))
            B.write_triple(out, T, stem=name)
        print("wrote", name)


if __name__ == "__main__":
    main()
