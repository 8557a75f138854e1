"""The persistent grid of the fused engine, counted in waves (select.inc grid_policy / ticket_policy), needs no device: the library's
self-test works it out for (registers, LDS bytes, batches, frames in flight) tuples on a 256-CU chip -- the 1080p path frame
alone and with two and four frames in flight (16, 12 and 8 waves per CU), frames with fewer tiles than waves (one workgroup per
batch, none left empty), a forced grid, a kernel the CU admits only once -- for workgroups of one, two and four waves, which must
come out as the same number of waves; and the ticket rule at its threshold."""


def test_grid_and_ticket_arithmetic(product_lib):
    from rayca_amd import lib
    lib.check(product_lib.rayca_hip_selftest())


def test_the_variant_library_is_built(product_lib):
    """build() leaves the 256-thread-workgroup variant beside the product library (tests/test_gpu_wave_blocks.py loads it)"""
    import os
    import __graft_entry__ as g
    assert os.path.isfile(g.VARIANT_LIB) and os.path.getmtime(g.VARIANT_LIB) >= os.path.getmtime(os.path.join(g.CSRC, "kernels.hip"))
