"""CPU oracle -- TEST INFRASTRUCTURE ONLY.

Restates the reference's algorithms for the hot path so the HIP path can be
checked on a box where /root/reference does not exist.  Only tests/, __graft_entry__.smoke()
and bench.py's cpu_baseline leg may import this package (and the experiment scripts under scripts/exp/: gemm_fuzz.py runs
gemm_ref, the float64 conv GEMM reference and error bound the GEMM tests use).  The product (artspeech_amd/) never does.
Pinning: every function here is checked against outputs of the reference itself, generated in the
build container by tests/golden/make_golden.py and committed under tests/golden/.  (gemm_ref restates no model: it is
plain float64 arithmetic of ConvGemmArgs, and tests/test_gemm_bound_cpu.py checks its bound against an emulation.)
"""
