// TEST DOUBLE'S COMPANION (tests/test_ramps_together.py): which k_chain instantiation the installed plan asks for.
#include "early_peek.h"

// PlanImage::chain_nq (fwgpu_plan_install.cpp chain_nq_for): bits 0..1 the tile in units of 64 frames, bit 2 a second recurrence stage,
// bit 3 the five-site stage logic
extern "C" int rmp_chain_nq(const fwgpu_ctx* c) { return c->chain_nq; }
