"""TEST-ONLY runner: `python -m tests.paths16_child gemm|attention` executes the 16-bit GEMM matrix / the 16-bit attention
forward list of tests/kernel_checks.py in THIS process and prints one JSON line.  DCLIP_ATTN16_TILED and DCLIP_ATTN16_NO_XQ
are read once into statics of the library, so tests/test_attention16_paths_gpu.py starts one fresh process per setting."""
import json
import os
import sys
import time

ONCE_READ = ("DCLIP_ATTN16_TILED", "DCLIP_ATTN16_NO_XQ")


def main(what: str) -> int:
    import torch
    from dclip_amd import _lib
    from tests import kernel_checks as kc

    t0 = time.time()
    lib = _lib.load()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    failed, sites, n = [], {}, 0
    if what == "gemm":
        for c in kc.gemm16_matrix():
            for k, v in kc.gemm16_env(c).items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
            n += 1
            try:
                fig = kc.run_gemm16_on_device(lib, c, dev, stream)
                sites[fig["site"]] = sites.get(fig["site"], 0) + 1
            except AssertionError as e:          # a wrong result is reported; a GPU fault ends the process, as it should
                failed.append(f"{kc.case16_id(c)}: {str(e)[:300]}")
    else:
        tiled = os.environ.get("DCLIP_ATTN16_TILED", "0") != "0"
        no_xq = os.environ.get("DCLIP_ATTN16_NO_XQ", "0") != "0"
        for c in kc.attn16_cases():
            if c.entry != "fwd":
                continue
            for data in ("select", "gauss"):
                n += 1
                try:
                    s = kc.build_attn16(c, dev, data)
                    site, = kc.launch_attn16(lib, s, stream)
                    torch.cuda.synchronize()
                    assert site == kc.expected_attn16_site(c, tiled=tiled, no_xq=no_xq), site
                    kc.verify_attn16(s, f"{kc.case_id(c)}-{data}")
                    sites[site] = sites.get(site, 0) + 1
                except AssertionError as e:
                    failed.append(f"{kc.case_id(c)}-{data}: {str(e)[:300]}")
    print(json.dumps({"cases": n, "failed": failed, "sites": sites, "seconds": round(time.time() - t0, 1),
                      "switches": {k: os.environ[k] for k in ONCE_READ if k in os.environ}}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
