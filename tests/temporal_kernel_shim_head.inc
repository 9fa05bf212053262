// What csrc/pt_temporal.hpp needs from HIP and from the headers it includes, for a HOST build of its two kernels
// (tests/test_temporal_kernel_host_cpu.py puts this file, the header's namespace ptd and temporal_kernel_shim_tail.inc into one
// translation unit): one "thread" at a time, blockDim = (1, 1), blockIdx = the pixel.  The arithmetic helpers are the ones of
// pt_math.hpp / pt_denoise.hpp / pt_denoise_guided.hpp, operation by operation.  ptd::TemporalArgs is the product's own
// (csrc/pt_denoise_host.hpp builds without HIP).
#include <cmath>
#include <cstddef>
#include <limits>
#include "pt_denoise_host.hpp"
#define __global__
#define __device__
#define __forceinline__ inline
struct f3 { float x,y,z; };
struct float4 { float x,y,z,w; };
struct uint4 { unsigned x,y,z,w; };
struct dim3 { unsigned x=1,y=1,z=1; };
static dim3 blockIdx, blockDim, threadIdx;
static inline f3 mk3(float x,float y,float z){ return {x,y,z}; }
static inline f3 ld3(const float* p){ return {p[0],p[1],p[2]}; }
static inline f3 operator-(f3 a,f3 b){ return {a.x-b.x,a.y-b.y,a.z-b.z}; }
static inline f3 operator+(f3 a,f3 b){ return {a.x+b.x,a.y+b.y,a.z+b.z}; }
static inline f3 operator*(f3 a,float s){ return {a.x*s,a.y*s,a.z*s}; }
static inline float inff(){ return std::numeric_limits<float>::infinity(); }
static inline bool finite1(float v){ return std::fabs(v) < inff(); }
static inline float4 make_float4(float x,float y,float z,float w){ return {x,y,z,w}; }
static inline float squaredDistance3( float4 a, float4 b ) { const float x = a.x - b.x, y = a.y - b.y, z = a.z - b.z; return ( x * x + y * y ) + z * z; }
