// Stand-alone host check of the validation code of dgtd_preprocess_batch and dgtd_preprocess: the job table is an exactly-sized heap
// block and every call is a refusal, so no launch is reached and no device is needed; an over-read of the table or a missed bound shows
// under the sanitizers.
//   P=<package>/csrc; hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       $P/preprocess_batch.hip $P/core.hip tools/preprocess_batch_hostcheck.cpp -o tools/_build/preprocess_batch_hostcheck && tools/_build/preprocess_batch_hostcheck
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../include/dgtd.h"

static int expect(int rc, int want, const char* what) {
  printf("%-28s rc=%d  %s\n", what, rc, rc ? dgtd_last_error() : "");
  return rc == want ? 0 : 1;
}

int main() {
  const int S = 64;
  int shapes[5][3] = {{97, 131, 3}, {20, 30, 1}, {1, 7, 1}, {50, 33, 3}, {300, 400, 1}};
  // exactly-sized heap table: an over-read of the table is an ASan error
  dgtd_preprocess_job* jobs = (dgtd_preprocess_job*)malloc(5 * sizeof(dgtd_preprocess_job));
  memset(jobs, 0, 5 * sizeof(dgtd_preprocess_job));
  int64_t p = 0, w = 0;
  auto al = [](int64_t v) { return (v + 15) & ~(int64_t)15; };
  auto ks = [&](int in) { return (in <= S ? 1 : (in + S - 1) / S) * 2 + 1; };
  for (int j = 0; j < 5; ++j) {
    dgtd_preprocess_job& b = jobs[j];
    b.H = shapes[j][0]; b.W = shapes[j][1]; b.C = shapes[j][2];
    b.out_sel = b.C == 3 ? 0 : 1; b.batch = j / 3; b.normalize = b.C == 3; b.flip = j & 1;
    b.src_off = p; p += al((int64_t)b.H * b.W * b.C);
    b.mid_off = w; w += al((int64_t)b.H * S * b.C);
    b.tab_h_off = w; w += al((int64_t)S * (2 + ks(b.W)) * 4);
    b.tab_v_off = w; w += al((int64_t)S * (2 + ks(b.H)) * 4);
  }
  int bad = 0;
  int64_t ws = dgtd_preprocess_batch_workspace(jobs, 5, S);
  printf("workspace %lld (own sum %lld)\n", (long long)ws, (long long)w);
  bad += ws != w;
  bad += dgtd_preprocess_batch_workspace(jobs, 0, S) != -1;
  float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  void* fake = (void*)(uintptr_t)0x1000;   // never dereferenced by the host code
  auto call = [&](int n, int64_t pb, int64_t wb) {
    return dgtd_preprocess_batch(fake, pb, (const dgtd_preprocess_job*)fake, jobs, n, fake, fake, fake, 2, S, mean, stdv, fake, wb, DGTD_F32, nullptr);
  };
  bad += expect(call(65536, p, w), 2, "too many jobs");
  bad += expect(call(0, p, w), 2, "no jobs");
  jobs[1].C = 2;            bad += expect(call(5, p, w), 2, "C = 2");            jobs[1].C = 1;
  jobs[3].tab_h_off += 8;   bad += expect(call(5, p, w), 2, "misaligned");       jobs[3].tab_h_off -= 8;
  bad += expect(call(5, p - 16, w), 2, "plane past the buffer");
  bad += expect(call(5, p, w - 16), 2, "table past the workspace");
  jobs[0].src_off = -16;    bad += expect(call(5, p, w), 2, "negative offset");  jobs[0].src_off = 0;
  jobs[0].H = jobs[0].W = 2147483647;  // H*W*C would wrap int64: refused by the bound on the sides, not by the byte arithmetic
  bad += expect(call(5, p, w), 2, "huge sides");  bad += dgtd_preprocess_batch_workspace(jobs, 5, S) != -1;  jobs[0].H = 97; jobs[0].W = 131;
  jobs[2].batch = 2;        bad += expect(call(5, p, w), 2, "batch index");      jobs[2].batch = 0;
  jobs[4].out_sel = 0;      bad += expect(call(5, p, w), 2, "C for output");     jobs[4].out_sel = 1;
  free(jobs);
  // the single-image entry: the same pipeline with its one job built on the host; every refusal comes before the first launch
  auto one = [&](int C, int S1, const float* m, const float* sd, dgtd_dtype dt) {
    return dgtd_preprocess(fake, fake, m, sd, fake, 97, 131, C, S1, 0, dt, nullptr);
  };
  bad += expect(one(0, S, nullptr, nullptr, DGTD_F32), 2, "single: C = 0");
  bad += expect(one(5, S, nullptr, nullptr, DGTD_F32), 2, "single: C = 5");
  bad += expect(one(3, 0, nullptr, nullptr, DGTD_F32), 2, "single: S = 0");
  bad += expect(one(3, S, mean, nullptr, DGTD_F32), 2, "single: mean without std");
  bad += expect(one(3, S, mean, stdv, DGTD_F64), 2, "single: bad dtype");
  // its workspace is the one-job layout of the batch entry; bad sizes give -1 (no division by S = 0)
  jobs = (dgtd_preprocess_job*)calloc(1, sizeof(dgtd_preprocess_job));
  jobs[0].H = 97; jobs[0].W = 131; jobs[0].C = 3;
  bad += dgtd_preprocess_workspace(97, 131, 3, S) != dgtd_preprocess_batch_workspace(jobs, 1, S);
  bad += dgtd_preprocess_workspace(97, 131, 3, 0) != -1;
  bad += dgtd_preprocess_workspace(97, 131, 5, S) != -1;
  free(jobs);
  printf(bad ? "FAILED %d\n" : "all refusals as expected\n", bad);
  return bad != 0;
}
