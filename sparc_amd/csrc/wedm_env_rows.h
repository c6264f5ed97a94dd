// wedm_env_rows.h — the scalar state rows of an environment, written once (included by wedm_device.h).
//
// A kernel holds most rows of wedm_f64_field, wedm_i32_field and wedm_i8_field (include/wedm_hip.h) in the members of its
// `Env`.  The lists below say, one line per register-held row and in the order load_env() requests them, which member holds
// which row and what a launch does with it.  load_env, store_env, load_env_inputs, store_env_after_*, the trace's env_*_row
// (wedm_device.h), the reset kernel's module masks and the rows wedm_bind_trace refuses (wedm_kernels.hip) are expansions of
// these lists; static_asserts tie the texts kept by hand to them.  Adding a state row: DESIGN.md section 3 has the recipe.
//
//   X(a, member, row, stage, role, owner)         (`a`: whatever the expansion hands through to X)
// member  the `Env` member.  Register and row convert by the cast between the member's type and the block's: float members
//         hold float32 values of float64 rows, key0 / key1 are the uint32 view of their rows, int8 rows sit in int32 registers.
// stage   which store of a single-microsecond launch has the row final (store_env_after_*, wedm_k_stream.h):
//           PRE_QUIET    after the scalar prelude, whichever prelude ran
//           PRE_GENERAL  after the scalar prelude, unless the whole wave took quiet_prelude_t, which never assigns these
//           EPILOGUE     after the scalar epilogue
//           NEVER        no step assigns the member and store_env() does not write the row: the resets and the caller do
// role    what a microsecond does with the value it finds in the row (load_env_inputs): IN reads it; OUT assigns it before
//         any use, so the single-microsecond kernel never loads the row; IN_FORCED is OUT except where the caller forces the
//         spark (wedm_params.disable_ignition); IN_KEEPSTEP is OUT except under wedm_params.keep_stepping_terminated
// owner   STATE: a field of the reference's EDMState, which every reset re-initialises.  MODULE: what the reference keeps in
//         its module objects, which a reset with reset_semantics 1 leaves alone (wedm_reset_kernel, reinit_env's
//         `keep_modules`; the oracle restates the set in reset_env_rows).
#pragma once

// the float64 rows held in double registers: what the reference keeps in EDMState and in its modules ...
#define WEDM_ENV_F64_DOUBLES(X, a) \
    X(a, wp,             WEDM_F_WORKPIECE_POS,  PRE_GENERAL, IN,          STATE)  \
    X(a, x,              WEDM_F_WIRE_POS,       EPILOGUE,    IN,          STATE)  \
    X(a, v,              WEDM_F_WIRE_VEL,       EPILOGUE,    IN,          STATE)  \
    X(a, prev_a,         WEDM_F_PREV_ACCEL,     EPILOGUE,    IN,          MODULE) \
    X(a, debris,         WEDM_F_DEBRIS_VOLUME,  PRE_QUIET,   IN,          MODULE) \
    X(a, rho,            WEDM_F_DEBRIS_DENSITY, PRE_QUIET,   IN,          STATE)  \
    X(a, flow,           WEDM_F_FLOW,           PRE_GENERAL, IN,          MODULE) \
    X(a, last_gap,       WEDM_F_LAST_GAP,       PRE_GENERAL, IN,          MODULE) \
    X(a, last_rho,       WEDM_F_LAST_DENSITY,   PRE_GENERAL, IN,          MODULE) \
    X(a, wire_last_flow, WEDM_F_WIRE_LAST_FLOW, PRE_GENERAL, IN,          MODULE) \
    X(a, V,              WEDM_F_VOLTAGE,        PRE_QUIET,   IN,          STATE)  \
    X(a, I,              WEDM_F_CURRENT,        PRE_QUIET,   IN_FORCED,   STATE)  \
    X(a, y,              WEDM_F_SPARK_Y,        PRE_QUIET,   IN,          STATE)  \
    X(a, last_crater,    WEDM_F_LAST_CRATER,    PRE_QUIET,   OUT,         STATE)  \
    X(a, cavity,         WEDM_F_CAVITY,         PRE_QUIET,   OUT,         STATE)  \
    X(a, tdelta,         WEDM_F_TARGET_DELTA,   PRE_GENERAL, IN,          STATE)  \
    X(a, tvolt,          WEDM_F_TARGET_VOLTAGE, PRE_GENERAL, IN,          STATE)  \
    X(a, on,             WEDM_F_ON_TIME,        PRE_GENERAL, IN,          STATE)  \
    X(a, off,            WEDM_F_OFF_TIME,       PRE_GENERAL, IN,          STATE)  \
    X(a, tpos,           WEDM_F_TARGET_POS,     NEVER,       IN,          STATE)  \
    X(a, unwind,         WEDM_F_UNWIND_VEL,     NEVER,       IN,          STATE)
// ... the running sums of the driver's statistics, also doubles ...
#define WEDM_ENV_F64_SUMS(X, a) \
    X(a, vacc,           WEDM_F_VOLT_ACC,       EPILOGUE,    IN,          STATE)
// ... and those held as the float32 values they are (the wire module's convection coefficients and its monitor)
#define WEDM_ENV_F64_FLOATS(X, a) \
    X(a, h_base,         WEDM_F_H_BASE,         PRE_GENERAL, IN,          MODULE) \
    X(a, h_zone,         WEDM_F_H_ZONE,         PRE_GENERAL, IN,          MODULE) \
    X(a, tmax,           WEDM_F_TMAX,           EPILOGUE,    IN_KEEPSTEP, STATE)
#define WEDM_ENV_F64(X, a) WEDM_ENV_F64_DOUBLES(X, a) WEDM_ENV_F64_SUMS(X, a) WEDM_ENV_F64_FLOATS(X, a)

#define WEDM_ENV_I32(X, a) \
    X(a, time,           WEDM_I_TIME,             EPILOGUE,    IN,        STATE)  \
    X(a, tss,            WEDM_I_SINCE_SERVO,      EPILOGUE,    IN,        STATE)  \
    X(a, tsov,           WEDM_I_SINCE_OPEN_V,     EPILOGUE,    IN,        STATE)  \
    X(a, tsi,            WEDM_I_SINCE_IGNITION,   EPILOGUE,    IN,        STATE)  \
    X(a, tse,            WEDM_I_SINCE_SPARK_END,  EPILOGUE,    IN,        STATE)  \
    X(a, dur,            WEDM_I_SPARK_DUR,        PRE_QUIET,   IN,        STATE)  \
    X(a, rnd_rem,        WEDM_I_RANDOM_SHORT_REM, PRE_GENERAL, IN,        MODULE) \
    X(a, deb_rem,        WEDM_I_DEBRIS_SHORT_REM, PRE_GENERAL, IN,        MODULE) \
    X(a, tcrit,          WEDM_I_TIME_CRITICAL,    EPILOGUE,    IN,        STATE)  \
    X(a, mode,           WEDM_I_CURRENT_MODE,     PRE_GENERAL, IN,        STATE)  \
    X(a, episode,        WEDM_I_EPISODE,          NEVER,       IN,        STATE)  \
    X(a, key0,           WEDM_I_KEY_LO,           NEVER,       IN,        STATE)  \
    X(a, key1,           WEDM_I_KEY_HI,           NEVER,       IN,        STATE)  \
    X(a, sparks,         WEDM_I_SPARK_COUNT,      PRE_GENERAL, IN,        MODULE)

// X_DONE: row DONE is the one row whose stored value is not simply its member (done_row(), wedm_device.h), so its line goes
// to a macro of its own; an expansion that reads only the columns passes the same macro twice.
#define WEDM_ENV_I8(X, X_DONE, a) \
    X(a, state,          WEDM_B_SPARK_STATE,      PRE_QUIET,   IN,        STATE)  \
    X(a, is_short,       WEDM_B_IS_SHORT,         PRE_QUIET,   IN_FORCED, STATE)  \
    X(a, broken,         WEDM_B_WIRE_BROKEN,      EPILOGUE,    IN,        STATE)  \
    X(a, reached,        WEDM_B_TARGET_REACHED,   EPILOGUE,    IN,        STATE)  \
    X_DONE(a, done,      WEDM_B_DONE,             EPILOGUE,    IN,        STATE)  \
    X(a, ctrl,           WEDM_B_CTRL_STEP,        PRE_QUIET,   OUT,       STATE)  \
    X(a, err,            WEDM_B_ERROR,            PRE_GENERAL, IN,        STATE)

// The state rows that NO `Env` member holds: X(row, owner, why the registers cannot answer for it).  They live in memory
// only: load_env / store_env pass them by, and a trace sample, taken from the registers, has no value for them.
#define WEDM_UNHELD_F64(X) X(WEDM_F_VOLT_SUM, STATE, "VOLT_SUM is published at control steps only")          // control_step_outputs()
#define WEDM_UNHELD_I32(X) X(WEDM_I_TIME_HI, STATE, "TIME_HI is maintained at the end of a launch only")     // store_time_hi()
#define WEDM_UNHELD_I8(X) X(WEDM_B_MODE_CACHED, MODULE, "MODE_CACHED is set in memory by the latching step") // scalar_prelude()

// ---- selecting lines by a column: every tag is a bit, a set of tags is their OR, and WEDM_HAS(set, stage, role, owner) says
// at compile time whether one of a line's three tags is in the set
namespace wedm {
enum : uint32_t {
    ROW_PRE_QUIET = 1u << 0, ROW_PRE_GENERAL = 1u << 1, ROW_EPILOGUE = 1u << 2, ROW_NEVER = 1u << 3,  // stage
    ROW_IN = 1u << 4, ROW_OUT = 1u << 5, ROW_IN_FORCED = 1u << 6, ROW_IN_KEEPSTEP = 1u << 7,          // role
    ROW_STATE = 1u << 8, ROW_MODULE = 1u << 9,                                                        // owner
    ROW_STORED = ROW_PRE_QUIET | ROW_PRE_GENERAL | ROW_EPILOGUE, ROW_ALL = ROW_IN | ROW_OUT | ROW_IN_FORCED | ROW_IN_KEEPSTEP,
};
#define WEDM_HAS(set, stage, role, owner) (((ROW_##stage | ROW_##role | ROW_##owner) & (set)) != 0)
// the same columns as masks over the rows of a block (bit r: row r), and the un-held rows
#define WEDM_ROW_BIT(set, m, row, stage, role, owner) | (WEDM_HAS(set, stage, role, owner) ? 1u << (row) : 0u)
#define WEDM_F64_ROWS(set) (0u WEDM_ENV_F64(WEDM_ROW_BIT, set))
#define WEDM_I32_ROWS(set) (0u WEDM_ENV_I32(WEDM_ROW_BIT, set))
#define WEDM_I8_ROWS(set) (0u WEDM_ENV_I8(WEDM_ROW_BIT, WEDM_ROW_BIT, set))
#define WEDM_UNHELD_BIT(row, owner, why) | 1u << (row)
#define WEDM_UNHELD_MODULE_BIT(row, owner, why) | (ROW_##owner == ROW_MODULE ? 1u << (row) : 0u)

// Every row of a block has exactly one home.  (Two lines for one row cannot compile: env_*_row would have two equal cases.)
#define WEDM_CHECK_HOMES(B, count) \
    static_assert((WEDM_##B##_ROWS(ROW_ALL) | (0u WEDM_UNHELD_##B(WEDM_UNHELD_BIT))) == (1u << (count)) - 1u && \
                  (WEDM_##B##_ROWS(ROW_ALL) & (0u WEDM_UNHELD_##B(WEDM_UNHELD_BIT))) == 0, "every " #B " state row needs exactly one home: " \
                  "a line of WEDM_ENV_" #B " or an entry of WEDM_UNHELD_" #B " (wedm_env_rows.h)")
WEDM_CHECK_HOMES(F64, WEDM_F64_COUNT);
WEDM_CHECK_HOMES(I32, WEDM_I32_COUNT);
WEDM_CHECK_HOMES(I8, WEDM_I8_COUNT);
// store_env(), store_env_after_* and load_env_inputs() expand one column with one tag per line: their groups cannot overlap or
// leave a line out.  The tag that can still go wrong is NEVER, which silently leaves a row unpersisted: stated a second time.
static_assert(WEDM_F64_ROWS(ROW_NEVER) == ((1u << WEDM_F_TARGET_POS) | (1u << WEDM_F_UNWIND_VEL)) && WEDM_I8_ROWS(ROW_NEVER) == 0 &&
              WEDM_I32_ROWS(ROW_NEVER) == ((1u << WEDM_I_EPISODE) | (1u << WEDM_I_KEY_LO) | (1u << WEDM_I_KEY_HI)),
              "stage NEVER is for the rows that no step assigns (target position, unwinding velocity, episode, RNG key): "
              "store_env() and the single-microsecond kernel's store_env_after_* would not persist any other row marked so");
}  // namespace wedm
