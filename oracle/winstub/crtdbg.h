/* oracle/winstub/crtdbg.h — TEST INFRASTRUCTURE ONLY.
 *
 * Stand-in of our own for the debug-runtime header: _ASSERT counts the conditions that do not hold,
 * per source line, and goes on as a release build would.  The glue that includes the encoder hands
 * the counts out; the tests read them, a tripped assertion is a finding and never an abort.
 */
#ifndef AC3MI_WINSTUB_CRTDBG_H
#define AC3MI_WINSTUB_CRTDBG_H
#define WINSTUB_ASSERT_SITES 16
static int winstub_assert_trips;                            /* all sites together */
static int winstub_assert_site[WINSTUB_ASSERT_SITES][2];    /* { source line, trips there } */
static inline void winstub_assert_trip(int line)
{
    winstub_assert_trips++;
    for (int i = 0; i < WINSTUB_ASSERT_SITES; i++) {
        if (winstub_assert_site[i][0] == 0) winstub_assert_site[i][0] = line;
        if (winstub_assert_site[i][0] == line) { winstub_assert_site[i][1]++; return; }
    }
}
#define _ASSERT(cond) ((cond) ? (void)0 : winstub_assert_trip(__LINE__))
#endif
