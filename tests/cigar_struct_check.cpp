// The public record of the compact result format is 24 bytes, six 32-bit fields in the documented order (valign_hip.h alone).
#include <stddef.h>
#include <stdio.h>

#include "valign_hip.h"

static_assert(sizeof(valign_hip_aln) == 24, "valign_hip_aln is 24 bytes");
static_assert(offsetof(valign_hip_aln, read_begin) == 0 && offsetof(valign_hip_aln, read_end) == 4 && offsetof(valign_hip_aln, ref_begin) == 8 &&
                  offsetof(valign_hip_aln, ref_end) == 12 && offsetof(valign_hip_aln, score) == 16 && offsetof(valign_hip_aln, n_ops) == 20,
              "field order of valign_hip_aln");

int main() {
    int (*device_entry)(valign_hip_engine *, int, long long, const void *, const void *, int, void *, void *, int, void *) = &valign_hip_align_cigar_device;
    int (*host_entry)(valign_hip_engine *, int, int, const char *const *, const char *const *, int, valign_hip_aln *, uint32_t *, long long,
                      long long *, long long *, int) = &valign_hip_align_cigar_host;
    printf("cigar struct ok %d\n", (int)(device_entry != nullptr && host_entry != nullptr));
    return 0;
}
