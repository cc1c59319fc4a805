"""Worker of the sharded BGEN test: launched once per rank by torch.distributed.run (tests/test_gpu_bgen_sharded.py).  Every
rank streams its block of variants (dist.read_bgen_shard) onto the SAME GPU (the test box has one), the ranks talk over gloo;
each rank writes its block's numerators and its view of the column-sharded fit."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mendeliht_amd import dist as D                         # noqa: E402


def main(out_path, bgen, pheno, k):
    rank, world, _ = D.init_from_env(backend="gloo")
    x, off, p_global, samples, chrom, pos, ids, ref, alt = D.read_bgen_shard(bgen)
    np.save(f"{out_path}.r{rank}.npy", x.export())
    y = np.loadtxt(pheno)
    res = D.fit_iht_sharded(y, x, None, col_offset=off, p_global=p_global, k=k, verbose=False)
    nz = np.flatnonzero(res.beta)
    json.dump(dict(world=world, rank=rank, off=off, p=x.p, p_global=p_global, denom=x.denom, ids=ids, n_samples=len(samples),
                   support=nz.tolist(), beta=res.beta[nz].tolist(), iter=int(res.iter), logl=res.logl,
                   logl_trace=res.trace["logl"].tolist()), open(f"{out_path}.r{rank}.json", "w"))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]))
