"""The holders the host API owns its device memory through (csrc/gq_host_res.h), without a GPU: a stand-alone program instantiates them over a
malloc-backed memory policy that counts its live blocks, refuses a second free and can be told to fail its k-th allocation."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / 'gym_quadruped_amd' / 'csrc'

PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <gq_host_res.h>

struct FakeMem {
  static std::set<void*> live;
  static int allocs, frees, bad_frees, fail_at; /* fail_at: the allocation (counted from 1 after arm()) that fails; 0: none */
  static void arm(int k) { allocs = frees = 0; fail_at = k; }
  static hipError_t alloc(void** p, size_t bytes) {
    if (++allocs == fail_at) return hipErrorOutOfMemory; /* like hipMalloc: the out-pointer stays untouched */
    *p = std::malloc(bytes ? bytes : 1);
    std::memset(*p, 0xa5, bytes);
    live.insert(*p);
    return hipSuccess;
  }
  static void free(void* p) {
    if (!live.erase(p)) { bad_frees++; return; } /* a second free, or of a block that never was */
    frees++;
    std::free(p);
  }
  static hipError_t zero(void* p, size_t bytes) { std::memset(p, 0, bytes); return hipSuccess; }
};
std::set<void*> FakeMem::live;
int FakeMem::allocs = 0, FakeMem::frees = 0, FakeMem::bad_frees = 0, FakeMem::fail_at = 0;
using B = gq::Buf<float, FakeMem>;

static int failed = 0;
#define CHECK(name, cond) do { const bool ok_ = (cond); std::printf("%s %s\n", name, ok_ ? "ok" : "FAILED"); failed += !ok_; } while (0)

int main() {
  {
    B a;
    FakeMem::arm(0);
    bool ok = a.ensure(10, true) == hipSuccess && a.get() && a.count() == 10 && FakeMem::live.size() == 1;
    for (int i = 0; ok && i < 10; i++) ok = a.get()[i] == 0.0f;
    float* first = a.get();
    ok = ok && a.ensure(4, false) == hipSuccess && a.get() == first && a.count() == 10 && FakeMem::allocs == 1; /* large enough: kept */
    CHECK("ensure_keeps_and_zeroes", ok);
    FakeMem::arm(1);
    ok = a.ensure(20, false) != hipSuccess && a.get() == nullptr && a.count() == 0;
    ok = ok && FakeMem::frees == 1 && FakeMem::live.empty() && FakeMem::bad_frees == 0; /* the old block went first, once */
    a.reset();                                                                          /* ... and an empty holder frees nothing */
    CHECK("failed_grow_leaves_empty", ok && FakeMem::frees == 1 && FakeMem::bad_frees == 0);
    FakeMem::arm(0);
    CHECK("grow_after_failure", a.ensure(20, false) == hipSuccess && a.count() == 20 && FakeMem::live.size() == 1);
  }
  CHECK("scope_exit_frees", FakeMem::live.empty() && FakeMem::bad_frees == 0);
  {
    B a; gq::Buf<double, FakeMem> b;
    FakeMem::arm(2);
    bool ok = gq::ensure_both(a, 7, b, 21, false) != hipSuccess && !a.get() && !b.get() && a.count() == 0 && b.count() == 0 && FakeMem::live.empty();
    FakeMem::arm(1);
    ok = ok && gq::ensure_both(a, 7, b, 21, false) != hipSuccess && !a.get() && !b.get() && FakeMem::live.empty();
    CHECK("group_failure_leaves_nothing", ok && FakeMem::bad_frees == 0);
    FakeMem::arm(0);
    CHECK("group_success_fills_both", gq::ensure_both(a, 7, b, 21, false) == hipSuccess && a.count() == 7 && b.count() == 21 && FakeMem::live.size() == 2);
  }
  {
    B a, c;
    FakeMem::arm(0);
    bool ok = a.ensure(3, false) == hipSuccess && c.ensure(5, false) == hipSuccess;
    float* pa = a.get();
    B m(std::move(a));
    ok = ok && !a.get() && a.count() == 0 && m.get() == pa && m.count() == 3;
    c = std::move(m); /* the target's own block is released, the source is left empty */
    ok = ok && !m.get() && m.count() == 0 && c.get() == pa && c.count() == 3 && FakeMem::live.size() == 1 && FakeMem::frees == 1;
    CHECK("move_leaves_source_empty", ok);
  }
  CHECK("live_at_exit_is_zero", FakeMem::live.empty() && FakeMem::bad_frees == 0);
  return failed ? 1 : 0;
}
'''


@pytest.fixture(scope='module')
def report(tmp_path_factory):
    """name -> 'ok' / 'FAILED' of every check the program makes (its exit status says the same once more)"""
    d = tmp_path_factory.mktemp('host_res')
    (d / 'res.hip').write_text(PROGRAM)
    subprocess.run([os.environ.get('HIPCC', 'hipcc'), '--offload-arch=gfx950', '-O1', '-std=c++17', '-I', str(CSRC), str(d / 'res.hip'), '-o', str(d / 'res')], check=True)
    r = subprocess.run([str(d / 'res')], capture_output=True, text=True)
    out = dict(line.split() for line in r.stdout.splitlines())
    assert (r.returncode == 0) == all(v == 'ok' for v in out.values()), r.stdout + r.stderr
    return out


def test_ensure_keeps_a_large_enough_block_and_zero_fills_on_request(report):
    assert report['ensure_keeps_and_zeroes'] == 'ok'


def test_failed_grow_leaves_the_holder_empty_and_frees_the_old_block_once(report):
    assert report['failed_grow_leaves_empty'] == 'ok' and report['grow_after_failure'] == 'ok'


def test_group_allocation_leaves_nothing_behind_when_a_member_fails(report):
    assert report['group_failure_leaves_nothing'] == 'ok' and report['group_success_fills_both'] == 'ok'


def test_move_leaves_the_source_empty(report):
    assert report['move_leaves_source_empty'] == 'ok'


def test_nothing_is_live_at_exit(report):
    assert report['scope_exit_frees'] == 'ok' and report['live_at_exit_is_zero'] == 'ok'
