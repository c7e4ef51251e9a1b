// Stand-alone host check of the validation code of dgtd_predict_maps: the job table is an exactly-sized heap block and every call is a
// refusal, so no launch is reached and no device is needed; an over-read of the table or a missed bound shows under the sanitizers.
//   P=<package>/csrc; hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       $P/predict_maps.hip $P/core.hip tools/predict_maps_hostcheck.cpp -o tools/_build/predict_maps_hostcheck && tools/_build/predict_maps_hostcheck
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../include/dgtd.h"

static int expect(int rc, int want, const char* what) {
  printf("%-28s rc=%d  %s\n", what, rc, rc ? dgtd_last_error() : "");
  return rc == want ? 0 : 1;
}

int main() {
  const int B = 3, S = 64, N = 5;
  int sizes[N][2] = {{97, 131}, {1, 7}, {64, 64}, {3, 1}, {300, 500}};
  // exactly-sized heap table: an over-read of the table is an ASan error
  dgtd_predict_job* jobs = (dgtd_predict_job*)malloc(N * sizeof(dgtd_predict_job));
  memset(jobs, 0, N * sizeof(dgtd_predict_job));
  int64_t end = 0;
  for (int j = 0; j < N; ++j) {
    dgtd_predict_job& b = jobs[j];
    b.out_off = (end + 15) & ~(int64_t)15;
    b.H = sizes[j][0]; b.W = sizes[j][1]; b.batch = j % B;
    end = b.out_off + (int64_t)b.H * b.W;
  }
  int bad = 0;
  bad += sizeof(dgtd_predict_job) != 32;
  const int64_t ws = dgtd_predict_maps_workspace(N);
  printf("workspace %lld for %d jobs\n", (long long)ws, N);
  bad += ws < 8 * N || (ws & 15) != 0;
  bad += dgtd_predict_maps_workspace(0) != -1;
  bad += dgtd_predict_maps_workspace(65536) != -1;
  void* fake = (void*)(uintptr_t)0x1000;   // never dereferenced by the host code
  auto call = [&](int n, int64_t out_bytes, int dt = DGTD_F32, int normalize = 0, int64_t wsb = 1 << 20, int batch = B) {
    return dgtd_predict_maps(fake, (dgtd_dtype)dt, batch, S, (const dgtd_predict_job*)fake, jobs, n, fake, out_bytes, normalize, fake, wsb, nullptr);
  };
  bad += expect(call(65536, end), 2, "too many jobs");
  bad += expect(call(0, end), 2, "no jobs");
  bad += expect(call(-1, end), 2, "negative job count");
  bad += expect(call(N, end, DGTD_F64), 2, "fp64 logits");
  bad += expect(call(N, end, 7), 2, "unknown dtype");
  bad += expect(call(N, end, DGTD_F32, 2), 2, "unknown normalize");
  bad += expect(call(N, end, DGTD_BF16, 1, ws - 8), 2, "workspace too small");
  bad += expect(call(N, end - 1), 2, "last map past the buffer");
  bad += expect(call(N, 0), 2, "empty output");
  jobs[1].H = 0;                  bad += expect(call(N, end), 2, "H = 0");               jobs[1].H = 1;
  jobs[1].W = (1 << 24) + 1;      bad += expect(call(N, end), 2, "W above 2^24");        jobs[1].W = 7;
  jobs[0].H = jobs[0].W = 2147483647;  // H*W stays inside int64 only because the sides are bounded first
  bad += expect(call(N, end), 2, "huge sides");                                          jobs[0].H = 97; jobs[0].W = 131;
  jobs[3].out_off += 8;           bad += expect(call(N, end), 2, "misaligned offset");   jobs[3].out_off -= 8;
  jobs[0].out_off = -16;          bad += expect(call(N, end), 2, "negative offset");     jobs[0].out_off = 0;
  jobs[2].batch = B;              bad += expect(call(N, end), 2, "batch = B");           jobs[2].batch = -1;
  bad += expect(call(N, end), 2, "batch = -1");                                          jobs[2].batch = 2;
  bad += expect(call(N, end, DGTD_F32, 0, 1 << 20, 2), 2, "batch index with B = 2");
  for (int r = 0; r < 3; ++r) { jobs[4].reserved[r] = 1; bad += expect(call(N, end), 2, "reserved field"); jobs[4].reserved[r] = 0; }
  free(jobs);
  printf(bad ? "FAILED %d\n" : "all refusals as expected\n", bad);
  return bad != 0;
}
