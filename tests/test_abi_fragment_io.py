"""Host side of imf_fragment_io.ahead_stream: the ctypes mirror against the library's own sizeof, the new field's place at the
end of the struct (a zero-filled caller built against the previous header stays valid), the header's declaration, and the bounds
of the static rule.  No GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fragment_io_mirror_has_the_librarys_size_and_ahead_stream_is_its_last_field():
    from imfnet_amd import _lib
    L = _lib.lib()
    assert L.imf_abi_sizeof_fragment_io() == C.sizeof(_lib.FragmentIO)
    names = [f[0] for f in _lib.FragmentIO._fields_]
    assert names[-1] == "ahead_stream" and names[-3:-1] == ["inputs_event", "reuse_event"]
    f = _lib.FragmentIO.ahead_stream
    assert f.offset + f.size == C.sizeof(_lib.FragmentIO) and f.size == C.sizeof(C.c_void_p)
    assert not _lib.FragmentIO().ahead_stream                                   # zero-filled: one chain


def test_header_declares_ahead_stream_last_and_the_size_query():
    with open(os.path.join(ROOT, "include", "imfnet_hip.h")) as fh:
        h = fh.read()
    body = h[h.index("typedef struct imf_fragment_io"):h.index("} imf_fragment_io;")]
    members = re.findall(r"^\s*(?:const\s+)?[A-Za-z_0-9]+\s*\*?\s*\*?([a-z_0-9]+(?:\[\d+\])?(?:,\s*\*?[a-z_0-9]+)*);", body, re.M)
    assert members[-1] == "ahead_stream" and "reuse_event" in members[-2]
    assert "size_t imf_abi_sizeof_fragment_io(void);" in h


def test_encoder_ahead_rule_is_static_and_within_the_chain():
    from imfnet_amd import _lib
    L = _lib.lib()
    assert L.imf_fragment_ahead_forwards() >= 0
    if "IMF_ENCODER_AHEAD" in os.environ:
        return
    for variant in (0, 3, 6):
        for n_items in (1, 2, 4, 8):
            n = L.imf_resunet_encoder_ahead(variant, n_items)
            assert 0 <= n <= 13 and n == L.imf_resunet_encoder_ahead(variant, n_items)
