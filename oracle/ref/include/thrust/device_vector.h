/* Host stand-in: included by the reference, nothing from it is used on the
 * pinned paths.  TEST INFRASTRUCTURE ONLY. */
#pragma once
