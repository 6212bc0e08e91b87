"""Host-side check of csrc/weight_schema.h (no GPU, no library): the strict state-dict match every
<family>_load_weights runs, compiled into a stand-alone program under the address and
undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cs566-project-lightglue_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <string>
#include <vector>

#include "weight_schema.h"

static void run(const char* label, const lg::WeightSchema& s, int n, const char* const* names,
                const float* const* tensors, const int64_t* numels) {
  std::vector<int> src;
  std::string err;
  if (s.match(n, names, tensors, numels, src, err)) {
    std::printf("%s|ok|", label);
    for (size_t k = 0; k < src.size(); ++k) std::printf("%s%d", k ? "," : "", src[k]);
    std::printf("\n");
  } else {
    std::printf("%s|error|%s\n", label, err.c_str());
  }
}

int main() {
  lg::WeightSchema s;
  s.add("a.weight", 6);
  s.add("a.bias", 2);
  s.add("b.weight", 4);
  std::printf("schema|%d|%s:%lld,%s:%lld,%s:%lld|%d,%d,%d,%d\n", s.size(), s.name(0).c_str(), (long long)s.numel(0),
              s.name(1).c_str(), (long long)s.numel(1), s.name(2).c_str(), (long long)s.numel(2), s.find("a.weight"),
              s.find("a.bias"), s.find("b.weight"), s.find("c.weight"));
  static float a[6], b[2], c[4], d[1];
  {  // shuffled order: src is the permutation
    const char* n[] = {"b.weight", "a.weight", "a.bias"};
    const float* t[] = {c, a, b};
    const int64_t k[] = {4, 6, 2};
    run("shuffled", s, 3, n, t, k);
  }
  {
    const char* n[] = {"a.weight", "a.bias", "b.weight", "c.weight"};
    const float* t[] = {a, b, c, d};
    const int64_t k[] = {6, 2, 4, 1};
    run("extra", s, 4, n, t, k);
  }
  {
    const char* n[] = {"a.weight", "a.bias", "a.bias", "b.weight"};
    const float* t[] = {a, b, b, c};
    const int64_t k[] = {6, 2, 2, 4};
    run("duplicate", s, 4, n, t, k);
  }
  {
    const char* n[] = {"a.weight", "a.bias", "b.weight"};
    const float* t[] = {a, b, c};
    const int64_t k[] = {6, 2, 3};
    run("numel", s, 3, n, t, k);
  }
  const char* all[] = {"a.weight", "a.bias", "b.weight"};
  const float* all_t[] = {a, b, c};
  const int64_t all_k[] = {6, 2, 4};
  for (int miss = 0; miss < 3; ++miss) {  // each one of the three keys missing
    const char* n[2];
    const float* t[2];
    int64_t k[2];
    for (int i = 0, j = 0; i < 3; ++i)
      if (i != miss) {
        n[j] = all[i];
        t[j] = all_t[i];
        k[j++] = all_k[i];
      }
    run(("missing" + std::to_string(miss)).c_str(), s, 2, n, t, k);
  }
  {
    const char* n[] = {"a.weight", nullptr, "b.weight"};
    run("null_name", s, 3, n, all_t, all_k);
  }
  {
    const float* t[] = {a, b, nullptr};
    run("null_tensor", s, 3, all, t, all_k);
  }
  run("empty_empty", lg::WeightSchema(), 0, nullptr, nullptr, nullptr);
  run("empty_dict", s, 0, nullptr, nullptr, nullptr);
  return 0;
}
"""

EXPECTED = {
    "schema": ["3", "a.weight:6,a.bias:2,b.weight:4", "0,1,2,-1"],
    "shuffled": ["ok", "1,2,0"],
    "extra": ["error", "unexpected key in state_dict: c.weight"],
    "duplicate": ["error", "duplicate key: a.bias"],
    "numel": ["error", "size mismatch for b.weight: expected 4 got 3"],
    "missing0": ["error", "missing key in state_dict: a.weight"],
    "missing1": ["error", "missing key in state_dict: a.bias"],
    "missing2": ["error", "missing key in state_dict: b.weight"],
    "null_name": ["error", "null tensor at index 1"],
    "null_tensor": ["error", "null tensor at index 2"],
    "empty_empty": ["ok", ""],
    "empty_dict": ["error", "missing key in state_dict: a.weight"],
}


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_weight_schema_match_under_sanitizers(tmp_path):
    src = tmp_path / "schema.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "schema"
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stderr == ""  # no sanitizer report
    got = {}
    for line in run.stdout.splitlines():
        label, *rest = line.split("|")
        got[label] = rest
    assert got == EXPECTED
