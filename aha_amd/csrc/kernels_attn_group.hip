// Draft-and-verify decode attention: the rows of ONE sequence in one pass over its KV pages.
//
//   attn_decode_group_kernel   block (kv head, split, group): attn_decode_group_body (attn_group_body.h) on one entry of the group table.
//                              The rows' K/V are in their slots already (kv_append_rows_kernel, kernels_batch.hip, in the launch before);
//                              every row gets the bits attn_decode_rows_kernel gives it.
//   attn_group_plan            the host rule that cuts a step's row table into groups, used by the model's step and the op-level entry.
//
// bf16 pages, head dim 128.  A KV8 model keeps attn_decode_rows_kv8_kernel.
#include <hip/hip_runtime.h>

#include <unordered_map>

#include "attn_group_body.h"
#include "common.h"
#include "kernels.h"

namespace aha {

namespace {

// one wave per SIMD: the accumulators of ATTN_GROUP_T tiles next to a page's K and V fragments need more than 256 registers
__global__ __launch_bounds__(256, 1) void attn_decode_group_kernel(AttnDecodeBatchArgs b, const int32_t* group_tab, int part_rows) {
  __shared__ __attribute__((aligned(16))) char smem[ATTN_GROUP_LDS];
  attn_decode_group_body<ATTN_GROUP_T>(b, group_tab + (int64_t)blockIdx.z * ATTN_GROUP_WORDS, part_rows, smem, (int)blockIdx.x, (int)blockIdx.y);
}

}  // namespace

int attn_group_rows_cap(int g) { return attn_group_cap(g); }

// Groups of a step's rows, in table order: a row joins the open group of its sequence (equal GEN_ROW_PAGE0) whose last row is one token
// shorter and has the same split count, while that group has room for another row (attn_group_rows_cap); every other row opens a group.
// So a run is cut where nsplit changes and where a block is full, and a row without a neighbour is a group of one.  Rows of a group need
// not be adjacent in the table (the engine puts every request's own row in front of all draft rows).
// mode (aha_hip_debug_rows_group): 0 = no groups (the caller launches attn_decode_rows_kernel), 1 = by plan, 2 = always.  The plan
// (profiles/attn_group.md): not at g = 16, where a tile holds one row and no MFMA column is shared, and only in a step whose longest row
// has ATTN_GROUP_PLAN_MIN_KV tokens -- measured faster at 8192 (step 3.6 -> 2.7 ms at one 0.6B sequence with 15 drafts), slower at 512 .. 640
// (1.73 -> 2.03 ms: four tiles one after the other on a page per wave, where the row-by-row launch spreads them over 16 blocks); the
// lengths between were not measured.
// -> the number of groups, `out` holding ATTN_GROUP_WORDS words each; *max_split the largest split count, *kv_tokens the groups' longest
// rows summed (what the launch reads from the pages).
int attn_group_plan(const int32_t* row_tab, int rows, int g, int mode, std::vector<int32_t>& out, int* max_split, double* kv_tokens) {
  out.clear();
  if (max_split) *max_split = 1;
  if (kv_tokens) *kv_tokens = 0;
  if (mode == 0 || rows <= 0 || g < 1 || g > 16 || (mode == 1 && g == 16)) return 0;
  if (mode == 1) {
    int longest = 0;
    for (int r = 0; r < rows; ++r) longest = std::max(longest, (int)row_tab[(size_t)r * GEN_ROW_WORDS + GEN_ROW_KVLEN]);
    if (longest < ATTN_GROUP_PLAN_MIN_KV) return 0;
  }
  const int cap = attn_group_cap(g);
  std::unordered_map<uint64_t, int> open;   // (page0, kv_len the next row must have) -> group
  int n = 0;
  for (int r = 0; r < rows; ++r) {
    const int32_t* t = row_tab + (size_t)r * GEN_ROW_WORDS;
    const uint64_t key = ((uint64_t)(uint32_t)t[GEN_ROW_PAGE0] << 32) | (uint32_t)t[GEN_ROW_KVLEN];
    int gi = -1;
    const auto it = open.find(key);
    if (it != open.end()) {
      const int32_t* e = out.data() + (size_t)it->second * ATTN_GROUP_WORDS;
      if (e[ATTN_GROUP_NSPLIT] == t[GEN_ROW_NSPLIT] && e[ATTN_GROUP_COUNT] < cap) gi = it->second;
      open.erase(it);
    }
    if (gi < 0) {
      gi = n++;
      out.resize((size_t)n * ATTN_GROUP_WORDS, 0);
      int32_t* e = out.data() + (size_t)gi * ATTN_GROUP_WORDS;
      e[ATTN_GROUP_NSPLIT] = t[GEN_ROW_NSPLIT];
      e[ATTN_GROUP_PAGE0] = t[GEN_ROW_PAGE0];
      e[ATTN_GROUP_KVLEN] = t[GEN_ROW_KVLEN];
      e[ATTN_GROUP_CTR] = t[GEN_ROW_CTR];
    }
    int32_t* e = out.data() + (size_t)gi * ATTN_GROUP_WORDS;
    const int j = e[ATTN_GROUP_COUNT]++;
    e[ATTN_GROUP_ROW0 + j] = r;
    e[ATTN_GROUP_CTRROW0 + j] = t[GEN_ROW_CTRROW];
    open[key + 1] = gi;   // the same page0, one token more
  }
  for (int gi = 0; gi < n; ++gi) {
    const int32_t* e = out.data() + (size_t)gi * ATTN_GROUP_WORDS;
    if (max_split) *max_split = std::max(*max_split, (int)e[ATTN_GROUP_NSPLIT]);
    if (kv_tokens) *kv_tokens += e[ATTN_GROUP_KVLEN] + e[ATTN_GROUP_COUNT] - 1;
  }
  return n;
}

bool attn_group_shape_ok(const AttnDecodeBatchArgs& b, int rows) {
  return b.nh > 0 && b.kvh > 0 && b.nh % b.kvh == 0 && b.nh / b.kvh <= 16 && (size_t)rows * b.max_nsplit * b.nh * 128 * 4 < ((size_t)1 << 31) &&
         (size_t)rows * (b.nh + 2 * b.kvh) * 128 < ((size_t)1 << 31);
}

void launch_attn_decode_group(const AttnDecodeBatchArgs& b, const int32_t* group_tab, int groups, int rows, int max_nsplit_groups, hipStream_t st) {
  if (groups <= 0) return;
  hipLaunchKernelGGL(attn_decode_group_kernel, dim3((unsigned)b.kvh, (unsigned)max_nsplit_groups, (unsigned)groups), dim3(256), 0, st, b, group_tab,
                     rows);
}

}  // namespace aha
