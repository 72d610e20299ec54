"""CPU: awr_conv_args.pool_out serves the plain / two-tensor 1x1 launches through the field the fused pair already had -- the struct keeps its
size (no new field), and the header, the ABI's documentation, states the new rule."""
import ctypes as C
import os
import re

from test_abi import REPO, lib  # noqa: F401  (fixture)


def test_conv_args_keeps_its_size(lib):
    # the formula tests/test_abi.py pins (padding before w_split; stat_slots, stat_slot_base; in2; Cin1 + padding; partial; split_k, split_max; bnr_act;
    # bnr2_y, bnr2_coef, stats2; w2, bias2; N1, N1x; in_bnb_y, in_bnb_coef; accum + padding; in_split; pool_out; out_nt + padding)
    assert C.sizeof(lib.ConvArgs) == 12 * 8 + 17 * 4 + 4 * 76 + 4 + 8 + 2 * 4 + 8 + 8 + 8 + 2 * 4 + 8 + 3 * 8 + 2 * 8 + 2 * 4 + 2 * 8 + 2 * 4 + 8 + 8 + 8
    assert lib.ConvArgs.pool_out.size == 8 and lib.ConvArgs.out_nt.offset == lib.ConvArgs.pool_out.offset + 8


def test_header_documents_the_pooled_1x1_form():
    text = open(os.path.join(REPO, "include", "awr_hip.h")).read()
    m = re.search(r"float\*\s*pool_out;(.*?)\n\s*int out_nt;", text, flags=re.S)
    assert m, "pool_out / out_nt not found in awr_conv_args"
    doc = " ".join(re.findall(r"/\*(.*?)\*/", m.group(1), flags=re.S))
    assert "fused pair only" not in doc
    for word in ("1x1", "in2", "split-K", "LDS-DMA", "never left unwritten"):
        assert word in doc, word
