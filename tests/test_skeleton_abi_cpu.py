"""Argument checks of the skeleton entry points: they come before any HIP call, so they run without a GPU."""


def test_argument_errors_before_any_launch(lib_built):
    from drivescenegen_amd import _lib
    lib = _lib.load()
    a, b, c, d = 4096, 8192, 12288, 16384      # never dereferenced: every call below is refused first
    assert lib.dsg_thin_lut_u8(None, 1, 8, 8, b, 10, c, d, None) == -1 and b"NULL" in lib.dsg_last_error()
    assert lib.dsg_thin_lut_u8(a, 1, 8, 8, b, 10, a, d, None) == -1 and b"alias" in lib.dsg_last_error()
    for n, h, w, it in ((0, 8, 8, 10), (1, 0, 8, 10), (1, 8, -1, 10), (1, 8, 8, 0)):
        assert lib.dsg_thin_lut_u8(a, n, h, w, b, it, c, d, None) == -1 and b"bad dims" in lib.dsg_last_error()
    # the bit-packed image with its border and a byte per word must fit 64 KiB of LDS: 608 x 608 is the largest square multiple
    # of 32 that does (a shape that fits is launched, so only the GPU tests can show one accepted)
    for h, w in ((768, 768), (640, 640), (1, 1 << 20), (1 << 14, 1), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.dsg_thin_lut_u8(a, 1, h, w, b, 10, c, d, None) == -1 and b"does not fit" in lib.dsg_last_error(), (h, w)
    assert lib.dsg_skel_nodes_u8(None, 1, 8, 8, None, c, 4, d, None) == -1 and b"NULL" in lib.dsg_last_error()
    assert lib.dsg_skel_nodes_u8(a, 1, 8, 8, None, None, 4, d, None) == -1 and b"coords" in lib.dsg_last_error()
    assert lib.dsg_skel_nodes_u8(a, 1, 8, 8, None, c, -1, d, None) == -1
    assert lib.dsg_skel_nodes_u8(a, 1, 1 << 16, 1 << 16, None, c, 4, d, None) == -1 and b"bad dims" in lib.dsg_last_error()
    assert lib.dsg_skel_nodes_u8(a, 1, 8, 8, a, c, 4, d, None) == -1 and b"alias" in lib.dsg_last_error()
