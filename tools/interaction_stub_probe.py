#!/usr/bin/env python3
"""What are the interactions worth in a launch?  The real launch plans of RMAT-20 through the real step kernel (self-test build, one launch
per minibatch) with the interactions reduced to a stub -- f2v_test_interaction_stub: "rows gathered, one add each", results wrong -- against
the same kernel as it is.   usage: interaction_stub_probe.py [batch = 65536] [dim = 128] [option = 5] [rounds = 2]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
import force2vec_amd as F
from force2vec_amd import _lib

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
dim = int(sys.argv[2]) if len(sys.argv) > 2 else 128
option = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 2
rowptr, colids = bench.load_graph(20, 16, 1)
n = len(rowptr) - 1
nb = -(-n // batch)
T = _lib.selftest_lib()
MODES = ((0, "the kernel as it is"), (1, "neighbour interactions stubbed"), (3, "neighbour and sample interactions stubbed"))
print("RMAT-20, option %d, D = %d, batch %d; microseconds per launch (self-test build, best of 3 x 10 epochs)" % (option, dim, batch), flush=True)
for r in range(rounds):
    for mode, what in MODES:
        eng = F.Engine(rowptr, colids, dim, selftest=True)  # (a fresh engine per figure: a stubbed run leaves garbage embeddings)
        eng.srand(1)
        eng.init_embeddings(0)
        _lib.check(T.f2v_test_interaction_stub(eng._h, mode), T)
        eng.train(option, 6, batch)
        us = min(eng.train(option, 10, batch) / 10 for _ in range(3)) / nb * 1e6
        print("round %d  %-42s %.1f us" % (r, what + ":", us), flush=True)
        eng.close()
