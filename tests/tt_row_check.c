/* Host side of tests/test_tt_row_host.py: gcr_tt_row (gaussiancity_amd/csrc/gcr_tt_row.h, the header the device code
 * includes) for every NG in [lo, hi] -- one line per NG: the rows of b = 0 .. NG - 1. */
#include <stdio.h>
#include <stdlib.h>

#include "gcr_tt_row.h"

int main(int argc, char** argv) {
  const unsigned lo = argc > 1 ? (unsigned)atoi(argv[1]) : 1u, hi = argc > 2 ? (unsigned)atoi(argv[2]) : 512u;
  for (unsigned ng = lo; ng <= hi; ng++) {
    for (unsigned b = 0; b < ng; b++) printf(b ? " %u" : "%u", gcr_tt_row(b, ng));
    printf("\n");
  }
  return 0;
}
