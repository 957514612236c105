// cuda_runtime.h — TEST INFRASTRUCTURE ONLY (oracle/ref_shim).
//
// Stand-in for the CUDA header of that name, for compiling the reference's own CPU-emulation path
// (`#define CUDA 0`) with g++: in that mode the reference needs only the vector PODs, their make_*
// constructors, dim3 and the name cudaGraphicsResource. Nothing here runs on a GPU.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

struct uint3 { unsigned int x, y, z; };
struct uint4 { unsigned int x, y, z, w; };
struct int3 { int x, y, z; };
struct float3 { float x, y, z; };

static inline uint3 make_uint3(unsigned int x, unsigned int y, unsigned int z) { uint3 r = {x, y, z}; return r; }
static inline uint4 make_uint4(unsigned int x, unsigned int y, unsigned int z, unsigned int w) {
    uint4 r = {x, y, z, w};
    return r;
}
static inline int3 make_int3(int x, int y, int z) { int3 r = {x, y, z}; return r; }
static inline float3 make_float3(float x, float y, float z) { float3 r = {x, y, z}; return r; }

struct dim3 {
    unsigned int x, y, z;
    dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};

struct cudaGraphicsResource;
