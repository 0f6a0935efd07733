"""The command line's FASTQ record parser (faqcs_amd/csrc/cli/cli_parse.h: line_end, parse_range) without a GPU and without the GPU library:
tools/cli_parse_check.cpp under AddressSanitizer and UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_record_parser_under_the_sanitizers(tmp_path):
    """tools/cli_parse_check.cpp: the one parser of the streaming and the mapped reader as host C++ with AddressSanitizer and UBSan, the text
    and the buffer heap blocks of exactly the stated sizes.  Both line endings, a lone '\\r' in every line, every way a text can end inside a
    record, the five fastq.cpp:next_read messages, empty reads, N at either end, both grow rules of the arena, lines of 31 ... 65 bytes around
    the vector step of find_break; each as one range and cut at every record boundary, against a byte-by-byte restatement in the tool; and
    line_end against its two-memchr definition on every placement of '\\r' and '\\n' in lines of 0 ... 70 bytes.  The tool exits non-zero
    at the first difference and when a listed case never came up."""
    exe = str(tmp_path / "cli_parse_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tools", "cli_parse_check.cpp")], capture_output=True, timeout=600)
    if r.returncode != 0 and b"asan" in r.stderr.lower():
        pytest.skip("no sanitizer runtime in this image")
    assert r.returncode == 0, r.stderr.decode()
    r = subprocess.run([exe], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    assert b"every case equal to the restatement" in r.stdout
