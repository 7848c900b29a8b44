"""CPU test: the host half of the stage-test entries' input layer (csrc/stage_input.h: the pair and CSR checks, the padded read
and CIGAR buffers), built for the host with plain g++ (scripts/stage_input_host_check.cpp, which holds the cases and what it
expects of them) and run under the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'scripts', 'stage_input_host_check.cpp')


def test_stage_input_under_the_sanitizers(tmp_path):
    exe = tmp_path / 'stage_input_host_check'
    subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-o', str(exe), SRC], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr
    assert 'all expectations hold' in r.stdout
