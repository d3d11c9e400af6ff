"""The _pcm calls' per-call table against the parent commit's digests, on the CPU stand-in for the HIP runtime (tests/pcm_tables_cases.py)."""
import pcm_tables_cases as pt


def test_pcm_tables_emu(emu):
    pt.case_pcm_tables(emu, "emu", "host")
