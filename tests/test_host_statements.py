"""The host statements (faqcs_amd/csrc/faqcs_host.cpp: faqcs_parse_host, faqcs_render_host, faqcs_deflate_host, faqcs_bgzf_index_host,
faqcs_inflate_host) as a stand-alone program under AddressSanitizer and UBSan (tools/host_statements_check.cpp): buffers of exactly the
stated sizes, the chunked parse against the one-call parse, the render and the deflate / inflate round trips.  The GPU tests treat these
statements as the truth; this is where they are checked themselves.  Nothing here is loaded into the Python process."""
import gzip
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _example():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "example_1.fastq.gz"), "rb") as f:
        return f.read()


CASES = {
    "example_1": _example,
    "empty": lambda: b"",
    "one_read_no_final_newline": lambda: b"@r1 only\nACGTACGTAC\n+\nIIIIIHHHHH",
    "crlf": lambda: b"@r1\r\nACGTN\r\n+\r\nIIII#\r\n@r2\r\nGGC\r\n+r2\r\nHHH\r\n",
    "zero_length_read": lambda: b"@a\nACGT\n+\nIIII\n@empty\n\n+\n\n@b\nTTGCA\n+\nHHHHH\n",
    "first_and_last_base_N": lambda: b"@n1\nNACGTN\n+\n#IIII#\n@n2\nNN\n+\n##\n@n3\nN\n+\n#\n",
}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("host_statements") / "host_statements_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", path,
                        os.path.join(ROOT, "tools", "host_statements_check.cpp"), os.path.join(ROOT, "faqcs_amd", "csrc", "faqcs_host.cpp")],
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    return path


@pytest.mark.parametrize("name", list(CASES))
def test_host_statements_under_the_sanitizers(exe, tmp_path, name):
    text = CASES[name]()
    src = tmp_path / (name + ".fastq")
    src.write_bytes(text)
    r = subprocess.run([exe, str(src)], capture_output=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr).decode()[-2000:]
    assert r.stderr == b"", r.stderr.decode()[-2000:]
    out = r.stdout.decode()
    assert out.startswith("%d bytes, " % len(text)) and out.rstrip().endswith(": ok"), out
    if name != "crlf" and name != "one_read_no_final_newline":
        assert "render equal to the text" in out, out  # (the canonical files: the round trip was compared, not passed over)
