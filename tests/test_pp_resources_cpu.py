"""The persistent GEMM (gemm_pp.hip) counts its vector-memory operations by hand (s_waitcnt vmcnt(N) against the DMA ring):
a register spill would add scratch loads / stores the counts do not know about (and a drain of the ring in front of each
reload).  Compile every instantiation for gfx950 and require: no VGPR spill, no scratch, 128 KiB of LDS, two waves per SIMD."""
import os

import pytest

from micro_diffusion_amd import hip, native

HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_pp256_kernels_do_not_spill(tmp_path):
    res = native.resource_usage("gemm_pp.hip", hip.HIPCC_FLAGS, tmp_path / "pp.o")
    kernels = [k for k in res if "gemm_bf16_pp_kernel" in k]
    assert len(kernels) == 10, ("expected the 10 pp256 instantiations (NT: bf16, residual, dact, dact from the cached derivative; NN: bf16, gelu, "
                                f"gelu + cached derivative, residual, f32; TN: f32), found {len(kernels)}")
    for name in kernels:
        v = res[name]
        assert v["spill"] == 0, f"{name} spills VGPRs"
        assert v["scratch"] == 0, f"{name} uses scratch"
        assert v["lds"] == 131072, name
        assert v["occ"] == 2, name
