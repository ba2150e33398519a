// What the RDS block sync stage (rds_sync.hip) reads of a device link bank (rds.hip).
// Not part of the public ABI (include/sdr.h).
#pragma once
#include <cstdint>

struct sdr_ctx;
struct sdr_rds_links;

namespace sdrint {

struct RdsLinksView {
  sdr_ctx* ctx;
  int S;
  int64_t max_added;        // the most scanned bits one call can add to a stream
  const uint8_t* diff;      // the scanned rows of the last call, diff_stride bytes apart
  int64_t diff_stride;
  const int* added;         // [stream][2] = {C, L - C}: the last call added diff[C .. L); {0, 0} on a fault
};
RdsLinksView rds_links_view(const sdr_rds_links* l);

}  // namespace sdrint
