// Stand-alone host check of the validation code of dgtd_sod_metrics_ragged: the job table is an exactly-sized heap block and every call
// is a refusal, so no launch is reached and no device is needed; an over-read of the table or a missed bound shows under the sanitizers.
//   P=<package>/csrc; hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       $P/sod_metrics.hip $P/core.hip tools/sod_metrics_ragged_hostcheck.cpp -o tools/_build/sod_metrics_ragged_hostcheck && \
//       tools/_build/sod_metrics_ragged_hostcheck
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../include/dgtd.h"

static int expect(int rc, int want, const char* what) {
  printf("%-28s rc=%d  %s\n", what, rc, rc ? dgtd_last_error() : "");
  return rc == want ? 0 : 1;
}

int main() {
  const int N = 5;
  int sizes[N][2] = {{97, 131}, {1, 7}, {64, 64}, {3, 1}, {300, 500}};
  // exactly-sized heap table: an over-read of the table is an ASan error
  dgtd_predict_job* jobs = (dgtd_predict_job*)malloc(N * sizeof(dgtd_predict_job));
  memset(jobs, 0, N * sizeof(dgtd_predict_job));
  int64_t end = 0;
  for (int j = 0; j < N; ++j) {
    dgtd_predict_job& b = jobs[j];
    b.out_off = (end + 15) & ~(int64_t)15;
    b.H = sizes[j][0]; b.W = sizes[j][1]; b.batch = -7;   // ignored by this entry
    end = b.out_off + (int64_t)b.H * b.W;
  }
  int bad = 0;
  const int64_t ws = dgtd_sod_metrics_workspace(N);
  printf("workspace %lld for %d jobs\n", (long long)ws, N);
  bad += ws < 8224 * N;
  uint8_t* fake = (uint8_t*)(uintptr_t)0x1000;   // never dereferenced by the host code
  double out[4] = {-1.0, -2.0, -3.0, -4.0};      // the poison must survive every refusal
  auto call = [&](int n, int64_t bytes, const uint8_t* p = (const uint8_t*)(uintptr_t)0x1000, const uint8_t* g = (const uint8_t*)(uintptr_t)0x1000,
                  const dgtd_predict_job* dev = (const dgtd_predict_job*)(uintptr_t)0x1000, const dgtd_predict_job* host = nullptr, double* o = nullptr,
                  void* w = (void*)(uintptr_t)0x1000, bool null_host = false, bool null_out = false) {
    return dgtd_sod_metrics_ragged(p, g, bytes, dev, null_host ? nullptr : (host ? host : jobs), n, null_out ? nullptr : (o ? o : out), w, nullptr);
  };
  bad += expect(call(65536, end), 2, "too many jobs");
  bad += expect(call(0, end), 2, "no jobs");
  bad += expect(call(-1, end), 2, "negative job count");
  bad += expect(call(N, end, nullptr), 2, "null pred8");
  bad += expect(call(N, end, fake, nullptr), 2, "null gt8");
  bad += expect(call(N, end, fake, fake, nullptr), 2, "null device table");
  bad += expect(call(N, end, fake, fake, (const dgtd_predict_job*)fake, nullptr, nullptr, fake, true), 2, "null host table");
  bad += expect(call(N, end, fake, fake, (const dgtd_predict_job*)fake, nullptr, nullptr, fake, false, true), 2, "null out");
  bad += expect(call(N, end, fake, fake, (const dgtd_predict_job*)fake, nullptr, nullptr, nullptr), 2, "null workspace");
  bad += expect(call(N, end, fake + 8), 2, "misaligned pred8");
  bad += expect(call(N, end, fake, fake + 4), 2, "misaligned gt8");
  bad += expect(call(N, end - 1), 2, "last map past the buffer");
  bad += expect(call(N, 0), 2, "empty buffers");
  bad += expect(call(N, -5), 2, "negative byte count");
  jobs[1].H = 0;                  bad += expect(call(N, end), 2, "H = 0");               jobs[1].H = 1;
  jobs[1].W = -3;                 bad += expect(call(N, end), 2, "W < 0");               jobs[1].W = 7;
  jobs[1].W = (1 << 24) + 1;      bad += expect(call(N, end), 2, "W above 2^24");        jobs[1].W = 7;
  jobs[0].H = jobs[0].W = 2147483647;  // H*W stays inside int64 only because the sides are bounded first
  bad += expect(call(N, end), 2, "huge sides");
  jobs[0].H = 1 << 16; jobs[0].W = (1 << 15) + 1;
  bad += expect(call(N, (int64_t)1 << 40), 2, "H*W above 2^31");                         jobs[0].H = 97; jobs[0].W = 131;
  jobs[3].out_off += 8;           bad += expect(call(N, end), 2, "misaligned offset");   jobs[3].out_off -= 8;
  jobs[0].out_off = -16;          bad += expect(call(N, end), 2, "negative offset");     jobs[0].out_off = 0;
  jobs[4].out_off = INT64_MAX - 15;  // the bound is written so that offset + map is never formed
  bad += expect(call(N, end), 2, "offset near INT64_MAX");
  free(jobs);
  bad += !(out[0] == -1.0 && out[1] == -2.0 && out[2] == -3.0 && out[3] == -4.0);
  printf(bad ? "FAILED %d\n" : "all refusals as expected, out untouched\n", bad);
  return bad != 0;
}
