"""CPU: k_trace_fused reads its fifteen ray pointers from the kernel-argument segment at offsetof(FusedArgs, in) (kernels.h), so the
code objects of the last build must place every explicit argument where that struct places its member — as test_build_resources.py
checks LeadArgs for the persistent kernels."""
from test_build_resources import kernels  # noqa: F401  (the fixture: metadata of optable_amd/csrc/build/*.o)


def test_fused_kernel_argument_segment_is_laid_out_like_fused_args(kernels):  # noqa: F811
    fused = [k for k in kernels if "k_trace_fused" in k["name"]]
    assert len(fused) >= 40
    for k in fused:
        explicit = k["args"][:11]  # blob, unit, in, n, K, out, seg_count, counts, n_classes, pair, uniform
        assert len(explicit) == 11, (k["name"], len(k["args"]))
        assert explicit[0] == (0, 48) and explicit[2] == (56, 120), (k["name"], explicit[:3])
        at = 0
        for idx, (offset, size) in enumerate(explicit):
            align = 8 if size >= 8 else 4
            at = (at + align - 1) // align * align
            assert offset == at, (k["name"], idx, offset, at)
            at += size
        sizes = [s for _, s in explicit]
        assert sizes[1] in (4, 8) and sizes[3] == 8 and sizes[4] == 4 and sizes[5] in (112, 8), (k["name"], sizes)
        assert sizes[6:] == [8, 8, 4, 4, 4], (k["name"], sizes)  # seg_count, counts, n_classes, pair, uniform: the mask is the LAST argument
