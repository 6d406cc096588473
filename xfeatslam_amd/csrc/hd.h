// hd.h -- XFH_HD marks a function written ONCE and compiled for host and device (the *_math.h and *_layout.h headers, nodes_clamp.h, the lane-local
// pieces of search_common.hip.h), so that an entry point in a capi_*.cpp or a sanitizer program under tests/cpp runs the very lines the kernels run.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XFH_HD __host__ __device__ __forceinline__
#else
#define XFH_HD inline
#endif

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;
