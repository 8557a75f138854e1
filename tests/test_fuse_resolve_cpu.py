"""Without a device: rayca_hip_selftest holds fuse_resolve_rule (which path frames are one launch: the one-sample depth-1 frame of
the fused engine under NEE, and none of a counting frame, more samples, deeper paths, no direct sampler, the wavefront engine, a
caller's rays, the stack machine) and pick_kernel's table with the fused path instantiations -- GEN0, LAST and not STATS, every
other path tuple not reading `fused` (select.inc selftest_kernel_selection)."""
from rayca_amd import lib


def test_selftest_holds_the_rule_and_the_picker_rows(product_lib):
    lib.check(product_lib.rayca_hip_selftest())
