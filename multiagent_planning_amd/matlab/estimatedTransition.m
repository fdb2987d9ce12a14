function [pk,vk,ak,K_T_used,scene_status,log,est] = estimatedTransition(po,pf,prm,K_T_max,error_tol,trigger_p,trigger_v,reanchor,noise_p,noise_v,seed,wind,pushes,meas_p,meas_v,gain_p,gain_v,meas_seed)
% Measured state (no reference counterpart): feedbackTransition in which the planner does not know the tracking error but MEASURES it -- the rule
% include/dmpc_hip.h pins.  On every column the true deviation is seen through uniform sensor noise of half-widths meas_p (metres) and meas_v (m/s)
% from the stream meas_seed and blended into the planner's belief with the fixed gains gain_p, gain_v in (0, 1] (default 1: the estimate is the
% measurement).  The feedback rule decides its events on that estimate and re-initialises the planner to it; THE VEHICLE IS NEVER MOVED BY IT.
% po, pf, prm, K_T_max, error_tol, trigger_p, trigger_v, reanchor, noise_p, noise_v, seed, wind, pushes: as feedbackTransition takes them; a
% disturbance is not required (noise inside the trigger without one is the plain flight; noise beyond it makes false events).
% pk, vk, ak (3 x K_T_max x N_cmd), K_T_used, scene_status: as 'transition'; the histories hold the true states.
% log: feedbackTransition's struct; its dev_p_max, dev_v_max are the norms the events were decided on (of the estimate).
% est: a struct of the estimate's report -- err_p_max, err_v_max (1 x N_cmd: the largest estimation error) and their columns err_p_col, err_v_col
% (0-based), dev_p_max, dev_v_max (the largest TRUE tracking error) and dev_p_col, dev_v_col, and eh_p, eh_v (3 x N_cmd): the belief at the last column.
po = reshape(po,3,[]); pf = reshape(pf,3,[]);
if nargin < 8 || isempty(reanchor), reanchor = 1; end
if nargin < 9 || isempty(noise_p), noise_p = 0; end
if nargin < 10 || isempty(noise_v), noise_v = 0; end
if nargin < 11 || isempty(seed), seed = 0; end
if nargin < 12, wind = []; end
if nargin < 13, pushes = []; end
if nargin < 14 || isempty(meas_p), meas_p = 0; end
if nargin < 15 || isempty(meas_v), meas_v = 0; end
if nargin < 16 || isempty(gain_p), gain_p = 1; end
if nargin < 17 || isempty(gain_v), gain_v = 1; end
if nargin < 18 || isempty(meas_seed), meas_seed = 0; end
log = struct(); est = struct();
[pk,vk,ak,K_T_used,scene_status,log.event_count,log.event_first,log.event_last,log.dev_p_max,log.dev_p_col,log.dev_v_max,log.dev_v_col, ...
    log.xh_p,log.xh_v,log.e_p,log.e_v,est.err_p_max,est.err_p_col,est.err_v_max,est.err_v_col,est.dev_p_max,est.dev_p_col,est.dev_v_max, ...
    est.dev_v_col,est.eh_p,est.eh_v] = dmpc_mex('transition_estimated', prm, po, pf, K_T_max, error_tol, trigger_p, trigger_v, reanchor, ...
    noise_p, noise_v, seed, wind, pushes, meas_p, meas_v, gain_p, gain_v, meas_seed);
end
