"""TEST-ONLY runner: `python -m tests.gemm_paths_child` executes the integer GEMM matrix of tests/kernel_checks.py in THIS
process and prints one JSON line.  DCLIP_GEMM_DMA and DCLIP_GEMM_GROUP_M are read once into statics of the library, so
tests/test_gemm_paths_gpu.py starts one fresh process per setting."""
import json
import os
import sys
import time


def main() -> int:
    import torch
    from dclip_amd import _lib
    from tests import kernel_checks as kc

    t0 = time.time()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    dma = os.environ.get("DCLIP_GEMM_DMA", "1") != "0"
    failed, sites = [], {}
    cases = kc.integer_matrix()
    for c in cases:
        for k, v in kc.gemm_env(c).items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        try:
            fig = kc.run_gemm_on_device(lib, c, dev, stream, dma=dma)
            sites[fig["site"]] = sites.get(fig["site"], 0) + 1
        except AssertionError as e:          # a wrong result is reported; a GPU fault ends the process, as it should
            failed.append(f"{kc.case_id(c)}: {str(e)[:300]}")
    print(json.dumps({"cases": len(cases), "failed": failed, "sites": sites, "seconds": round(time.time() - t0, 1),
                      "switches": {k: v for k, v in os.environ.items() if k.startswith("DCLIP_GEMM_")
                                   and k not in ("DCLIP_GEMM_TILE", "DCLIP_GEMM_PLAN_TABLE")}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
