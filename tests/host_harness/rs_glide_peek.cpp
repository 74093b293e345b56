// TEST DOUBLE'S COMPANION (tests/test_rs_glide.py, tests/test_cmd_wire.py): the messages a host-only ctx keeps for nodes that no
// built plan holds yet, and nothing else.
#include "early_peek.h"
