"""the LDS-form set kernel at 1 % and 50 % selectivity, two calls each (run under rocprofv3 --pmc)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from midoridb_amd.dev import DeviceCtx
dev = DeviceCtx(0)
n = 100_000_000
rng = np.random.default_rng(5)
for sel in (0.01, 0.5):
    domain = int(round(1000 / sel))
    v = dev.gen_keys(n, 0, n, 7, domain)
    s = dev.make_set(rng.choice(domain, 1000, replace=False))
    for _ in range(2):
        print(sel, dev.filter([s.insn(0)], [(v, None, None)], n).numel())
    s.close()
    del v
dev.close()
