// Host-side pieces shared by the paged decode and prefill launchers.
#pragma once

// log2 of a power-of-two page size
inline int paged_page_shift(int page_size) {
  int page_shift = 0;
  while ((1 << page_shift) < page_size) ++page_shift;
  return page_shift;
}

// Runs LAUNCH(HD, G, FP8) with the compile-time constants of the runtime
// (hd, G, fp8), over the instantiated set hd in {64, 128} x G in {1, 2, 4, 8}
// x {bf16, fp8}. Outside that set the enclosing launcher returns -1.
#define KT_PAGED_CASE(hd, G, fp8, LAUNCH, HD_, G_) \
  if ((hd) == HD_ && (G) == G_) {                  \
    if (fp8)                                       \
      LAUNCH(HD_, G_, true);                       \
    else                                           \
      LAUNCH(HD_, G_, false);                      \
  } else
#define KT_PAGED_DISPATCH(hd, G, fp8, LAUNCH) \
  KT_PAGED_CASE(hd, G, fp8, LAUNCH, 64, 1)    \
  KT_PAGED_CASE(hd, G, fp8, LAUNCH, 64, 2)    \
  KT_PAGED_CASE(hd, G, fp8, LAUNCH, 64, 4)    \
  KT_PAGED_CASE(hd, G, fp8, LAUNCH, 64, 8)    \
  KT_PAGED_CASE(hd, G, fp8, LAUNCH, 128, 1)   \
  KT_PAGED_CASE(hd, G, fp8, LAUNCH, 128, 2)   \
  KT_PAGED_CASE(hd, G, fp8, LAUNCH, 128, 4)   \
  KT_PAGED_CASE(hd, G, fp8, LAUNCH, 128, 8)   \
  return -1
