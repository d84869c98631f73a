"""Host-bound ENQUEUE-COST probe (not a throughput figure): 1000 retrieve_batch steps of ONE query on a
4096-row dense + lexical index, a host clock around the loop that ends in a device synchronise.
    python scripts/enqueue_probe.py ROOT      (ROOT: the tree whose package is measured, e.g. a checkout
    of another commit; profiles/native_binding.md)"""
import json
import os
import sys
import time

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import triple_hybrid_rag_amd as T  # noqa: E402
from triple_hybrid_rag_amd import synth  # noqa: E402
from oracle import thr_oracle as O  # noqa: E402

assert os.path.dirname(T.__file__).startswith(root), T.__file__
torch.cuda.set_device(0)
n, d, nq, steps = 4096, 768, 1, 1000
x = synth.dense_rows(0, n, d)
q = synth.dense_queries(nq, d, n)
doc, term, tf = synth.lexical_rows(0, n, n)
csr = synth.build_lexical_csr(doc, term, tf, n, synth.vocab_size(n))
idf = O.bm25_idf(n, csr.df_local)
qt = synth.lexical_queries(nq, csr.df_local, 4)
idx = T.GpuIndex().set_dense(x).set_lexical(csr.rowptr, csr.post_doc, csr.post_tf, csr.doclen, idf, csr.sum_dl_local / n)
qd, qtd = torch.from_numpy(q).cuda(), torch.from_numpy(qt).cuda()
for _ in range(200):
    res = idx.retrieve_batch(qd, qtd, top_k=10)
torch.cuda.synchronize()
runs = []
for _ in range(3):
    t0 = time.perf_counter()
    for _ in range(steps):
        res = idx.retrieve_batch(qd, qtd, top_k=10)
    torch.cuda.synchronize()
    runs.append((time.perf_counter() - t0) / steps * 1e6)
print(json.dumps({"probe": "enqueue cost, us per retrieve_batch step (1 query, 4096 rows, dense + lexical)",
                  "package": os.path.dirname(T.__file__), "us_per_step": [round(r, 2) for r in runs],
                  "best_us_per_step": round(min(runs), 2), "ids": res.ids.cpu().numpy().tolist()}), flush=True)
