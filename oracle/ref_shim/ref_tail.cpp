// oracle/ref_shim/ref_tail.cpp -- TEST INFRASTRUCTURE ONLY.
//
// Compiles the tail of the reference's KGMT.cu (getR1, getR2, getCost, inGoalRegion)
// for the host.  The rest of that file needs thrust, cub and cuRAND, so the Makefile's
// `ref` target slices the file's #define lines and everything from the definition of
// getR1 to its end into oracle/_ref/kgmt_tail.inc (untracked, rebuilt from the
// reference tree) and this file includes the slice, unmodified.
// <math.h> gives the unqualified pow and sqrt the tail calls: under g++ pow(float, int)
// is the double overload, so inGoalRegion computes its distance in double.
#include <math.h>

#include "kgmt_tail.inc"
