/* oracle/winstub/windows.h — TEST INFRASTRUCTURE ONLY.
 *
 * Stand-in of our own for the one Win32 header the reference encoder includes.  The encoder uses
 * nothing of Win32; it only assumes the LLP64 data model of its compiler, where `long` has 32 bits
 * (its bit writer stores one `unsigned long` per 32 bits written).  The C library headers are
 * included first, so that their prototypes are seen with the platform's own `long`.
 */
#ifndef AC3MI_WINSTUB_WINDOWS_H
#define AC3MI_WINSTUB_WINDOWS_H
#include <stdio.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#define long int
#endif
