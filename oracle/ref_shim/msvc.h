// msvc.h — TEST INFRASTRUCTURE ONLY (oracle/ref_shim, force-included when oracle/Makefile's target
// ref_frame compiles the reference's CPU-emulation path with g++).
//
// The reference is MSVC code: Types.h spells its integer types __int32 / __int64. `long`, not
// `long long`, so that the reference's u64 is the same type as glm's and stays unambiguous where both
// namespaces are opened. u16 / u8 are used by reference files without a declaration in scope.
#pragma once
#define __int32 int
#define __int64 long
typedef unsigned short u16;
typedef unsigned char u8;
